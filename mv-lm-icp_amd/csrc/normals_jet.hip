// Jet-fitted normals (mvicp_fit_normals): the normal of mvicp_estimate_normals corrected by the slope of a height polynomial of degree 2 or 3
// fitted over its tangent plane (an osculating jet, Cazals & Pouget 2005), as a pure function of the stored bytes, bit for bit.  The contract
// is stated in include/mvicp.h; tests/jetref.py is its numpy form and its scalar-loop form.  DESIGN.md §3.16.
//
// One pass behind the internal self-mode knn_search, on the context's stream:
//   normals_jet<M>  one wave per point, lane t = entry t of the row, M = 6 or 10 monomials.  The PCA part is normals_pca.h's, the one
//                   mvicp_estimate_normals runs.  Then every lane holds its entry's scaled coordinates (X, Y, Z) in the frame (u, v, n) and its
//                   M monomials.  The Cholesky factorisation runs column by column, the forward solve with it: a column's M - j + 1 tree sums
//                   are formed together when the column is reached, the lanes SHARING the sums between them (scatter_tree_sum: the
//                   contract's tree, about a quarter of the shuffles of one butterfly per sum), and a readlane makes each wave-uniform for the
//                   arithmetic every lane then repeats.  A refused fit (too few points, h == 0, a failed pivot, a non-finite result) is a
//                   flag, not a branch: the arithmetic runs on and the PCA bytes are stored.  Every matrix index is a constant after
//                   unrolling.  lanes 0 .. 2 store the normal, lane 3 the curvature, lane 4 the count, lane 5 the fitted byte.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
#include "common.h"
#include "normals_pca.h"

namespace mvicp {

namespace {

constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
constexpr int pow2_ceil(int n) { int b = 1; while (b < n) b <<= 1; return b; }

// One step of the tree for W sums at once, across the lane bit X: of each pair (y[2i], y[2i+1]) a lane keeps the one its bit X selects, sends
// the other to its partner and adds what it receives -- y[u] <- y[2u] + y[2u+1] of the contract's tree for both sums, IEEE addition being
// commutative, with one shuffle where two butterflies take two.  W / 2 sums remain per lane.
template <int W, int X> __device__ __forceinline__ void scatter_step(double* y, int lane) {
  if constexpr (W > 1) {
    const bool up = (lane & X) != 0;
#pragma unroll
    for (int i = 0; i < W / 2; ++i) {
      const double keep = up ? y[2 * i + 1] : y[2 * i], send = up ? y[2 * i] : y[2 * i + 1];
      y[i] = __dadd_rn(keep, __shfl_xor(send, X, 64));
    }
    scatter_step<W / 2, 2 * X>(y, lane);
  }
}
// T of B sums (a power of two, <= 64) whose lane values are y[0 .. B-1]: lane l ends with T of sum l & (B - 1).  The first log2(B) levels of the
// tree are scatter steps, the rest the plain butterfly on the one value left.  y is used up.
template <int B> __device__ __forceinline__ double scatter_tree_sum(double (&y)[B], int lane) {
  scatter_step<B, 1>(y, lane);
  double v = y[0];
#pragma unroll
  for (int x = B; x < 64; x <<= 1) v = __dadd_rn(v, __shfl_xor(v, x, 64));
  return v;
}
// lane `src`'s value (src a constant) in every lane
__device__ __forceinline__ double lane_value(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// the largest of the 64 lanes' values (none is a NaN, none negative), in every lane
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { const double o = __shfl_xor(v, x, 64); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ bool finite(double v) { return fabs(v) < __builtin_huge_val(); }

// Column J of the Cholesky factorisation L (L[r][c], r >= c) with the forward solve y carried along as one more row.  The column's sums --
// G_JJ, G_rJ for r > J and r_J -- are formed here, together, by one scatter_tree_sum; lane e then holds the e-th of them.
template <int M, int J> __device__ __forceinline__ void jet_column(const double (&b)[M], double Z, int lane, double (&L)[M][M], double (&y)[M], bool& ok) {
  constexpr int N = M - J + 1, B = pow2_ceil(N);
  double t[B];
#pragma unroll
  for (int r = J; r < M; ++r) t[r - J] = __dmul_rn(b[J], b[r]);
  t[M - J] = __dmul_rn(b[J], Z);
#pragma unroll
  for (int e = N; e < B; ++e) t[e] = 0.0;
  const double sums = scatter_tree_sum<B>(t, lane);
  const double Gjj = lane_value(sums, 0);
  double s = Gjj;
#pragma unroll
  for (int q = 0; q < J; ++q) s = __dsub_rn(s, __dmul_rn(L[J][q], L[J][q]));
  ok = ok && s > __dmul_rn(0x1p-20, Gjj);
  const double Ljj = __dsqrt_rn(s);
  L[J][J] = Ljj;
#pragma unroll
  for (int r = J + 1; r < M; ++r) {
    s = lane_value(sums, r - J);
#pragma unroll
    for (int q = 0; q < J; ++q) s = __dsub_rn(s, __dmul_rn(L[r][q], L[J][q]));
    L[r][J] = __ddiv_rn(s, Ljj);
  }
  s = lane_value(sums, M - J);
#pragma unroll
  for (int q = 0; q < J; ++q) s = __dsub_rn(s, __dmul_rn(L[J][q], y[q]));
  y[J] = __ddiv_rn(s, Ljj);
  if constexpr (J + 1 < M) jet_column<M, J + 1>(b, Z, lane, L, y, ok);
}

template <int M>
__global__ __launch_bounds__(64 * kWavesPerBlock) void normals_jet_kernel(const double* __restrict__ pts, int n, int k, const int* __restrict__ cnt,
                                                                          const int* __restrict__ idx, double vx, double vy, double vz,
                                                                          double* __restrict__ nrm, double* __restrict__ curv, int* __restrict__ used,
                                                                          unsigned char* __restrict__ fitted) {
  // (one wave per point: saying so lets the point's own loads be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];   // <= k <= 64
  const double* pi = pts + 3 * (size_t)i;
  const double px = pi[0], py = pi[1], pz = pi[2];
  double d0, d1, d2, nx, ny, nz, cv;
  pca::row_offset(pts, idx, i, k, len, lane, px, py, pz, d0, d1, d2);
  pca::point_normal(d0, d1, d2, len, lane, px, py, pz, vx, vy, vz, nx, ny, nz, cv);
  bool ok = false;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0;
  if (len >= M) {   // (wave-uniform)
    // the tangent frame from n alone: w = e_a x n for the axis a of the smallest |n_a|, the first of equals
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const bool s1 = ay < ax;
    const bool s2 = az < (s1 ? ay : ax);
    const double w0 = s2 ? -ny : s1 ? nz : 0.0, w1 = s2 ? nx : s1 ? 0.0 : -nz, w2 = s2 ? 0.0 : s1 ? -nx : ny;
    const double lw = __dsqrt_rn(dot3(w0, w1, w2, w0, w1, w2));
    const double u0 = __ddiv_rn(w0, lw), u1 = __ddiv_rn(w1, lw), u2 = __ddiv_rn(w2, lw);
    const double v0 = __dsub_rn(__dmul_rn(ny, u2), __dmul_rn(nz, u1)), v1 = __dsub_rn(__dmul_rn(nz, u0), __dmul_rn(nx, u2)),
                 v2 = __dsub_rn(__dmul_rn(nx, u1), __dmul_rn(ny, u0));
    const double h = __dsqrt_rn(wave_max(dot3(d0, d1, d2, d0, d1, d2)));
    ok = !(h == 0.0);
    const bool in = lane < len;
    const double X = in ? __ddiv_rn(dot3(d0, d1, d2, u0, u1, u2), h) : 0.0, Y = in ? __ddiv_rn(dot3(d0, d1, d2, v0, v1, v2), h) : 0.0,
                 Z = in ? __ddiv_rn(dot3(d0, d1, d2, nx, ny, nz), h) : 0.0;
    double b[M];
    b[0] = in ? 1.0 : 0.0; b[1] = X; b[2] = Y;
    b[3] = __dmul_rn(X, X); b[4] = __dmul_rn(X, Y); b[5] = __dmul_rn(Y, Y);
    if constexpr (M == 10) { b[6] = __dmul_rn(b[3], X); b[7] = __dmul_rn(b[3], Y); b[8] = __dmul_rn(X, b[5]); b[9] = __dmul_rn(b[5], Y); }
    double L[M][M], y[M];
    jet_column<M, 0>(b, Z, lane, L, y, ok);
    // the back substitution down to a_1 (a_0, the height at the point, is not computed)
    double a[M];
#pragma unroll
    for (int m = M - 1; m >= 1; --m) {
      double s = y[m];
#pragma unroll
      for (int q = M - 1; q > m; --q) s = __dsub_rn(s, __dmul_rn(L[q][m], a[q]));
      a[m] = __ddiv_rn(s, L[m][m]);
    }
    g0 = __dsub_rn(__dsub_rn(nx, __dmul_rn(a[1], u0)), __dmul_rn(a[2], v0));
    g1 = __dsub_rn(__dsub_rn(ny, __dmul_rn(a[1], u1)), __dmul_rn(a[2], v1));
    g2 = __dsub_rn(__dsub_rn(nz, __dmul_rn(a[1], u2)), __dmul_rn(a[2], v2));
    const double lg = __dsqrt_rn(dot3(g0, g1, g2, g0, g1, g2));
    ok = ok && finite(g0) && finite(g1) && finite(g2) && finite(lg) && !(lg == 0.0);
    g0 = __ddiv_rn(g0, lg); g1 = __ddiv_rn(g1, lg); g2 = __ddiv_rn(g2, lg);
  }
  if (ok) { nx = g0; ny = g1; nz = g2; }
  if (lane < 3) nrm[3 * (size_t)i + lane] = lane == 0 ? nx : lane == 1 ? ny : nz;
  if (lane == 3) curv[i] = cv;
  if (lane == 4) used[i] = len;
  if (lane == 5) fitted[i] = ok ? 1 : 0;
}

}  // namespace

long long normals_fit(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2, const double* viewpoint, int degree) {
  c->nrm.drop_result();   // (the last result ends here; a failed call leaves none behind)
  const long long total = knn_search(c, f, nullptr, 0, 0, max_nn, radius, B2);
  if (total < 0) return total;
  const int n = f.n;
  if (n == 0) { c->nrm.rows = 0; c->nrm.has_fit = 1; return 0; }
  hipStream_t st = c->stream;
  const size_t N = (size_t)n;
  const size_t off_curv = align256(24 * N), off_used = off_curv + align256(8 * N), off_fit = off_used + align256(4 * N);
  MV_CHECK(c->nrm.dev.reserve(off_fit + align256(N)));
  c->nrm.nrm = reinterpret_cast<double*>(c->nrm.dev.p);
  c->nrm.curv = reinterpret_cast<double*>(c->nrm.dev.p + off_curv);
  c->nrm.used = reinterpret_cast<int*>(c->nrm.dev.p + off_used);
  c->nrm.fitted = reinterpret_cast<unsigned char*>(c->nrm.dev.p + off_fit);
  {
    // per point its position, count and index row, the 37 bytes it writes; per neighbour a position
    ProfScope ps(c, "normals_jet", (24.0 + 4.0 + 4.0 * max_nn + 37.0) * n + 24.0 * total);
    const dim3 grid((unsigned int)((N + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    if (degree == 2)
      hipLaunchKernelGGL(normals_jet_kernel<6>, grid, block, 0, st, f.pts, n, max_nn, c->knn.cnt, c->knn.idx, viewpoint[0], viewpoint[1], viewpoint[2],
                         c->nrm.nrm, c->nrm.curv, c->nrm.used, c->nrm.fitted);
    else
      hipLaunchKernelGGL(normals_jet_kernel<10>, grid, block, 0, st, f.pts, n, max_nn, c->knn.cnt, c->knn.idx, viewpoint[0], viewpoint[1], viewpoint[2],
                         c->nrm.nrm, c->nrm.curv, c->nrm.used, c->nrm.fitted);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipStreamSynchronize(st));
  c->nrm.rows = n; c->nrm.has_fit = 1;
  return n;
}

}  // namespace mvicp
