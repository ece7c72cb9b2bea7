// Jet-fitted normals (mvicp_fit_normals): the normal of mvicp_estimate_normals corrected by the slope of a height polynomial of degree 2 or 3
// fitted over its tangent plane (an osculating jet, Cazals & Pouget 2005), as a pure function of the stored bytes, bit for bit.  The contract
// is stated in include/mvicp.h; tests/jetref.py is its numpy form and its scalar-loop form.  DESIGN.md §3.16.
//
// One pass behind the internal self-mode knn_search, on the context's stream:
//   normals_jet<M>  one wave per point, lane t = entry t of the row, M = 6 or 10 monomials.  The PCA part is normals_pca.h's, the one
//                   mvicp_estimate_normals runs; the pieces of the fit are normals_jet.h's, which smooth.hip (mvicp_smooth_points) shares.
//                   Then every lane holds its entry's scaled coordinates (X, Y, Z) in the frame (u, v, n) and its M monomials.  The Cholesky factorisation runs column by column, the forward solve with it: a column's M - j + 1 tree sums
//                   are formed together when the column is reached, the lanes SHARING the sums between them (scatter_tree_sum: the
//                   contract's tree, about a quarter of the shuffles of one butterfly per sum), and a readlane makes each wave-uniform for the
//                   arithmetic every lane then repeats.  A refused fit (too few points, h == 0, a failed pivot, a non-finite result) is a
//                   flag, not a branch: the arithmetic runs on and the PCA bytes are stored.  Every matrix index is a constant after
//                   unrolling.  lanes 0 .. 2 store the normal, lane 3 the curvature, lane 4 the count, lane 5 the fitted byte.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
#include "common.h"
#include "normals_jet.h"
#include "normals_pca.h"

namespace mvicp {

namespace {

using namespace jet;

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
    const jet::Tangent f = jet::tangent_frame(nx, ny, nz);
    const double u0 = f.u0, u1 = f.u1, u2 = f.u2, v0 = f.v0, v1 = f.v1, v2 = f.v2;
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
  MV_CHECK(c->nrm.reserve_fit(N));
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
