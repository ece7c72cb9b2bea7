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
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.  The per-point part lives in normals_pca.h,
// which normals_jet.hip (mvicp_fit_normals) shares.
#include "common.h"
#include "normals_pca.h"

namespace mvicp {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int VT = 256;

__global__ __launch_bounds__(64 * kWavesPerBlock) void normals_pca_kernel(const double* __restrict__ pts, int n, int k, const int* __restrict__ cnt,
                                                                          const int* __restrict__ idx, double vx, double vy, double vz,
                                                                          double* __restrict__ nrm, double* __restrict__ curv, int* __restrict__ used) {
  // (one wave per point: saying so lets the point's own loads be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];   // <= k <= 64
  const double* pi = pts + 3 * (size_t)i;
  const double px = pi[0], py = pi[1], pz = pi[2];
  double d0, d1, d2, nx, ny, nz, cv;
  pca::row_offset(pts, idx, i, k, len, lane, px, py, pz, d0, d1, d2);
  pca::point_normal(d0, d1, d2, len, lane, px, py, pz, vx, vy, vz, nx, ny, nz, cv);
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
  c->nrm.drop_result();   // (the last result ends here; a failed call leaves none behind)
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
