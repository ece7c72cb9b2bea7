// Normals with curvature, oriented to a viewpoint (mvicp_estimate_normals): per point of one stored cloud the eigenvector of the smallest
// eigenvalue of the covariance of its neighbourhood, turned towards a viewpoint, and the surface variation l_min / (l0 + l1 + l2), as a
// pure function of the stored bytes, bit for bit.  The contract is stated in include/mvicp.h; tests/normref.py is its numpy form and its
// scalar-loop form.  DESIGN.md §3.14.
//
// The neighbourhoods are the rows of one internal knn_search (self mode, the max_nn nearest, within the radius if one is given, ordered by
// (dist2, original index)); a row is at most 64 long, one wave64.  One pass behind it, on the context's stream:
//   normals_pca  one wave per point, lane t = entry t of the row: the lane gathers p_j from the original-order points and forms the
//                offset d = p_j - p_i (lanes past the row carry +0.0); nine xor-butterfly sums across the wave (3 means, 6 moments) -- the
//                butterfly forms the pairwise tree y[u] <- y[2u] + y[2u+1] of the contract in every lane at once, because IEEE addition
//                is commutative -- then the 3 x 3 Jacobi iteration of the ISS contract with the vectors, on values every lane holds alike;
//                lanes 0 .. 2 store the normal, lane 3 the curvature, lane 4 the count.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
#include "common.h"

namespace mvicp {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kSweeps = 6;
constexpr int VT = 256;

// T(y): the sum of the 64 lanes' values in the order of the contract's tree, in every lane
__device__ __forceinline__ double tree_sum(double v) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) v = __dadd_rn(v, __shfl_xor(v, x, 64));
  return v;
}

// a 3 x 3 matrix in nine named registers: every index below is a template argument, so nothing is addressed at run time
struct M33 { double m00, m01, m02, m10, m11, m12, m20, m21, m22; };
template <int R, int C> __device__ __forceinline__ double& at(M33& m) {
  if constexpr (R == 0) { if constexpr (C == 0) return m.m00; else if constexpr (C == 1) return m.m01; else return m.m02; }
  else if constexpr (R == 1) { if constexpr (C == 0) return m.m10; else if constexpr (C == 1) return m.m11; else return m.m12; }
  else { if constexpr (C == 0) return m.m20; else if constexpr (C == 1) return m.m21; else return m.m22; }
}
// columns P, Q: (x[r][P], x[r][Q]) <- (c x[r][P] - s x[r][Q], s x[r][P] + c x[r][Q])
template <int R, int P, int Q> __device__ __forceinline__ void rot_cols(M33& x, double c, double s) {
  const double xp = at<R, P>(x), xq = at<R, Q>(x);
  at<R, P>(x) = __dsub_rn(__dmul_rn(c, xp), __dmul_rn(s, xq)); at<R, Q>(x) = __dadd_rn(__dmul_rn(s, xp), __dmul_rn(c, xq));
}
template <int R, int P, int Q> __device__ __forceinline__ void rot_rows(M33& x, double c, double s) {
  const double xp = at<P, R>(x), xq = at<Q, R>(x);
  at<P, R>(x) = __dsub_rn(__dmul_rn(c, xp), __dmul_rn(s, xq)); at<Q, R>(x) = __dadd_rn(__dmul_rn(s, xp), __dmul_rn(c, xq));
}
// one rotation of the ISS contract's Jacobi iteration (iss.hip jacobi_eigenvalues) on the pair (P, Q), with the vectors
template <int P, int Q> __device__ __forceinline__ void rotate(M33& A, M33& V) {
  const double apq = at<P, Q>(A);
  if (apq == 0.0) return;
  const double theta = __ddiv_rn(__dsub_rn(at<Q, Q>(A), at<P, P>(A)), __dmul_rn(2.0, apq));
  const double t = __ddiv_rn(theta >= 0 ? 1.0 : -1.0, __dadd_rn(fabs(theta), __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
  const double c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0))), s = __dmul_rn(t, c);
  rot_cols<0, P, Q>(A, c, s); rot_cols<1, P, Q>(A, c, s); rot_cols<2, P, Q>(A, c, s);   // A <- A J
  rot_rows<0, P, Q>(A, c, s); rot_rows<1, P, Q>(A, c, s); rot_rows<2, P, Q>(A, c, s);   // A <- J^T A
  rot_cols<0, P, Q>(V, c, s); rot_cols<1, P, Q>(V, c, s); rot_cols<2, P, Q>(V, c, s);   // V <- V J
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void normals_pca_kernel(const double* __restrict__ pts, int n, int k, const int* __restrict__ cnt,
                                                                          const int* __restrict__ idx, double vx, double vy, double vz,
                                                                          double* __restrict__ nrm, double* __restrict__ curv, int* __restrict__ used) {
  // (one wave per point: saying so lets the point's own loads be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];   // <= k <= 64
  const double* pi = pts + 3 * (size_t)i;
  const double px = pi[0], py = pi[1], pz = pi[2];
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  if (lane < len) {
    const double* pj = pts + 3 * (size_t)idx[(size_t)i * (size_t)k + lane];
    d0 = __dsub_rn(pj[0], px); d1 = __dsub_rn(pj[1], py); d2 = __dsub_rn(pj[2], pz);
  }
  double nx = 0.0, ny = 0.0, nz = 0.0, cv = 0.0;
  if (len >= 3) {   // (wave-uniform)
    const double c = (double)len;
    const double m0 = __ddiv_rn(tree_sum(d0), c), m1 = __ddiv_rn(tree_sum(d1), c), m2 = __ddiv_rn(tree_sum(d2), c);
    const bool in = lane < len;
    const double x0 = in ? __dsub_rn(d0, m0) : 0.0, x1 = in ? __dsub_rn(d1, m1) : 0.0, x2 = in ? __dsub_rn(d2, m2) : 0.0;
    const double c00 = tree_sum(__dmul_rn(x0, x0)), c01 = tree_sum(__dmul_rn(x0, x1)), c02 = tree_sum(__dmul_rn(x0, x2));
    const double c11 = tree_sum(__dmul_rn(x1, x1)), c12 = tree_sum(__dmul_rn(x1, x2)), c22 = tree_sum(__dmul_rn(x2, x2));
    M33 A = {c00, c01, c02, c01, c11, c12, c02, c12, c22}, V = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) { rotate<0, 1>(A, V); rotate<0, 2>(A, V); rotate<1, 2>(A, V); }
    const double a0 = A.m00, a1 = A.m11, a2 = A.m22;
    const bool b1 = a1 < a0;
    const double l1 = b1 ? a1 : a0;
    const bool b2 = a2 < l1;
    const double l = b2 ? a2 : l1;
    const double e0 = b2 ? V.m02 : b1 ? V.m01 : V.m00, e1 = b2 ? V.m12 : b1 ? V.m11 : V.m10, e2 = b2 ? V.m22 : b1 ? V.m21 : V.m20;
    const double nn = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)), __dmul_rn(e2, e2)));
    nx = __ddiv_rn(e0, nn); ny = __ddiv_rn(e1, nn); nz = __ddiv_rn(e2, nn);
    const double w0 = __dsub_rn(vx, px), w1 = __dsub_rn(vy, py), w2 = __dsub_rn(vz, pz);
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(nx, w0), __dmul_rn(ny, w1)), __dmul_rn(nz, w2));
    if (s < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double S = __dadd_rn(__dadd_rn(a0, a1), a2);
    if (l > 0.0 && S > 0.0) cv = __ddiv_rn(l, S);
  }
  if (lane < 3) nrm[3 * (size_t)i + lane] = lane == 0 ? nx : lane == 1 ? ny : nz;
  if (lane == 3) curv[i] = cv;
  if (lane == 4) used[i] = len;
}

// adoption: the result's normals into the frame's original-order and sorted arrays
__global__ __launch_bounds__(VT) void normals_adopt_kernel(const double* __restrict__ nrm, int n, const int* __restrict__ inv, double* __restrict__ nor,
                                                           double* __restrict__ snor) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  const size_t s = (size_t)inv[i];   // < n
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double v = nrm[3 * (size_t)i + a];
    nor[3 * (size_t)i + a] = v;
    snor[3 * s + a] = v;
  }
}

}  // namespace

long long normals_estimate(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2, const double* viewpoint) {
  c->nrm.rows = -1; c->nrm.frame = -1;   // (the last result ends here; a failed call leaves none behind)
  const long long total = knn_search(c, f, nullptr, 0, 0, max_nn, radius, B2);
  if (total < 0) return total;
  const int n = f.n;
  if (n == 0) { c->nrm.rows = 0; return 0; }
  hipStream_t st = c->stream;
  const size_t N = (size_t)n;
  const size_t off_curv = align256(24 * N), off_used = off_curv + align256(8 * N);
  MV_CHECK(c->nrm.dev.reserve(off_used + align256(4 * N)));
  c->nrm.nrm = reinterpret_cast<double*>(c->nrm.dev.p);
  c->nrm.curv = reinterpret_cast<double*>(c->nrm.dev.p + off_curv);
  c->nrm.used = reinterpret_cast<int*>(c->nrm.dev.p + off_used);
  {
    // per point its position, count and index row, the 36 bytes it writes; per neighbour a position
    ProfScope ps(c, "normals_pca", (24.0 + 4.0 + 4.0 * max_nn + 36.0) * n + 24.0 * total);
    hipLaunchKernelGGL(normals_pca_kernel, dim3((unsigned int)((N + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, f.pts, n, max_nn,
                       c->knn.cnt, c->knn.idx, viewpoint[0], viewpoint[1], viewpoint[2], c->nrm.nrm, c->nrm.curv, c->nrm.used);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipStreamSynchronize(st));
  c->nrm.rows = n;
  return n;
}

int normals_adopt(mvicp_ctx* c, FrameDev& f, const double* nrm) {
  hipLaunchKernelGGL(normals_adopt_kernel, dim3(grid_of(f.n, VT)), dim3(VT), 0, c->stream, nrm, f.n, f.grid.inv, f.nor, f.grid.snor);
  MV_HIP(hipGetLastError());
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
}

}  // namespace mvicp
