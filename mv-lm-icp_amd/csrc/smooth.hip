// Jet smoothing (mvicp_smooth_points): every point moved onto the height polynomial fitted through its neighbourhood, along its PCA normal
// (CGAL's jet_smooth_point_set, the unweighted form of moving least squares), and the mean and Gaussian curvature of that polynomial at the
// point, as a pure function of the stored bytes, bit for bit.  The contract is stated in include/mvicp.h; tests/smoothref.py is its numpy
// form and its scalar-loop form.  DESIGN.md §3.21.
//
// One pass behind the internal self-mode knn_search, on the context's stream:
//   jet_smooth<M>   one wave per point, lane t = entry t of the row, M = 6 or 10 monomials.  The PCA part is normals_pca.h's and the fit
//                   normals_jet.h's, the ones mvicp_fit_normals runs, with the back substitution continued by one row to a_0: column 0 of
//                   L is live until then anyway.  What follows -- the shift a_0 h, the projection and the curvatures from a_1 .. a_5 -- is
//                   some 40 wave-uniform operations that every lane repeats.  As in the fit a refusal is a flag, not a branch.  lanes 0 .. 5
//                   store mvicp_fit_normals' bytes (normal, curvature, count, fitted), lanes 6 .. 8 the point, lanes 9 .. 11 shift, H and
//                   K, lane 12 the moved byte.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
#include "common.h"
#include "normals_jet.h"
#include "normals_pca.h"

namespace mvicp {

namespace {

using namespace jet;

template <int M>
__global__ __launch_bounds__(64 * kWavesPerBlock) void jet_smooth_kernel(const double* __restrict__ pts, int n, int k, const int* __restrict__ cnt,
                                                                         const int* __restrict__ idx, double vx, double vy, double vz, double max_shift,
                                                                         double* __restrict__ nrm, double* __restrict__ curv, int* __restrict__ used,
                                                                         unsigned char* __restrict__ fitted, double* __restrict__ xyz,
                                                                         double* __restrict__ shift, double* __restrict__ Hout, double* __restrict__ Kout,
                                                                         unsigned char* __restrict__ moved) {
  // (one wave per point: saying so lets the point's own loads be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];   // <= k <= 64
  const double* pi = pts + 3 * (size_t)i;
  const double px = pi[0], py = pi[1], pz = pi[2];
  double d0, d1, d2, nx, ny, nz, cv;
  pca::row_offset(pts, idx, i, k, len, lane, px, py, pz, d0, d1, d2);
  pca::point_normal(d0, d1, d2, len, lane, px, py, pz, vx, vy, vz, nx, ny, nz, cv);
  bool ok = false, mv = false;
  double g0 = 0.0, g1 = 0.0, g2 = 0.0, x0 = px, x1 = py, x2 = pz, sh = 0.0, Hm = 0.0, Kg = 0.0;
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
    // the back substitution down to a_0, the height at the point
    double a[M];
#pragma unroll
    for (int m = M - 1; m >= 0; --m) {
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
    // the shift and the projection along the PCA normal
    const double ah = __dmul_rn(a[0], h);
    if (ok && finite(ah)) sh = ah;
    const double q0 = __dadd_rn(px, __dmul_rn(sh, nx)), q1 = __dadd_rn(py, __dmul_rn(sh, ny)), q2 = __dadd_rn(pz, __dmul_rn(sh, nz));
    mv = ok && finite(ah) && (max_shift <= 0.0 || fabs(sh) <= max_shift) && finite(q0) && finite(q1) && finite(q2);
    if (mv) { x0 = q0; x1 = q1; x2 = q2; }
    // the curvatures of z = a_1 X + a_2 Y + a_3 X2 + a_4 XY + a_5 Y2 + ... at the point, X and Y in units of h
    const double E = __dadd_rn(1.0, __dmul_rn(a[1], a[1])), G = __dadd_rn(1.0, __dmul_rn(a[2], a[2])), F = __dmul_rn(a[1], a[2]);
    const double w2 = __dadd_rn(E, __dmul_rn(a[2], a[2])), w = __dsqrt_rn(w2);
    const double zxx = __ddiv_rn(__dadd_rn(a[3], a[3]), h), zxy = __ddiv_rn(a[4], h), zyy = __ddiv_rn(__dadd_rn(a[5], a[5]), h);
    const double w3 = __dmul_rn(w2, w);
    const double Hv = __ddiv_rn(__dadd_rn(__dsub_rn(__dmul_rn(G, zxx), __dmul_rn(__dadd_rn(F, F), zxy)), __dmul_rn(E, zyy)), __dadd_rn(w3, w3));
    const double Kv = __ddiv_rn(__dsub_rn(__dmul_rn(zxx, zyy), __dmul_rn(zxy, zxy)), __dmul_rn(w2, w2));
    if (ok && finite(Hv) && finite(Kv)) { Hm = Hv; Kg = Kv; }
  }
  if (ok) { nx = g0; ny = g1; nz = g2; }
  if (lane < 3) nrm[3 * (size_t)i + lane] = lane == 0 ? nx : lane == 1 ? ny : nz;
  if (lane == 3) curv[i] = cv;
  if (lane == 4) used[i] = len;
  if (lane == 5) fitted[i] = ok ? 1 : 0;
  if (lane >= 6 && lane < 9) xyz[3 * (size_t)i + (lane - 6)] = lane == 6 ? x0 : lane == 7 ? x1 : x2;
  if (lane == 9) shift[i] = sh;
  if (lane == 10) Hout[i] = Hm;
  if (lane == 11) Kout[i] = Kg;
  if (lane == 12) moved[i] = mv ? 1 : 0;
}

}  // namespace

long long smooth_points(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2, const double* viewpoint, int degree, double max_shift) {
  c->nrm.drop_result();   // (the last result ends here; a failed call leaves none behind)
  const long long total = knn_search(c, f, nullptr, 0, 0, max_nn, radius, B2);
  if (total < 0) return total;
  const int n = f.n;
  if (n == 0) { c->nrm.rows = 0; c->nrm.has_fit = 1; c->nrm.has_smooth = 1; return 0; }
  hipStream_t st = c->stream;
  const size_t N = (size_t)n;
  NormalsStage& S = c->nrm;
  MV_CHECK(S.reserve_fit(N));
  const size_t off_shift = align256(24 * N), off_H = off_shift + align256(8 * N), off_K = off_H + align256(8 * N), off_moved = off_K + align256(8 * N);
  MV_CHECK(S.smo.reserve(off_moved + align256(N)));
  S.xyz = reinterpret_cast<double*>(S.smo.p);
  S.shift = reinterpret_cast<double*>(S.smo.p + off_shift);
  S.H = reinterpret_cast<double*>(S.smo.p + off_H);
  S.K = reinterpret_cast<double*>(S.smo.p + off_K);
  S.moved = reinterpret_cast<unsigned char*>(S.smo.p + off_moved);
  {
    // per point its position, count and index row, the 37 + 49 bytes it writes; per neighbour a position
    ProfScope ps(c, "jet_smooth", (24.0 + 4.0 + 4.0 * max_nn + 37.0 + 49.0) * n + 24.0 * total);
    const dim3 grid((unsigned int)((N + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    if (degree == 2)
      hipLaunchKernelGGL(jet_smooth_kernel<6>, grid, block, 0, st, f.pts, n, max_nn, c->knn.cnt, c->knn.idx, viewpoint[0], viewpoint[1], viewpoint[2],
                         max_shift, S.nrm, S.curv, S.used, S.fitted, S.xyz, S.shift, S.H, S.K, S.moved);
    else
      hipLaunchKernelGGL(jet_smooth_kernel<10>, grid, block, 0, st, f.pts, n, max_nn, c->knn.cnt, c->knn.idx, viewpoint[0], viewpoint[1], viewpoint[2],
                         max_shift, S.nrm, S.curv, S.used, S.fitted, S.xyz, S.shift, S.H, S.K, S.moved);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipStreamSynchronize(st));
  S.rows = n; S.has_fit = 1; S.has_smooth = 1;
  return n;
}

}  // namespace mvicp
