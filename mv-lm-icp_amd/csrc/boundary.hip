// Boundary points of one stored cloud (mvicp_boundary, mvicp_boundary_select): a point is on the boundary when, seen in its tangent plane, its
// neighbours leave an angular gap of at least theta = acos(cos_gap), as a pure function of the stored bytes, bit for bit.  The contract is
// stated in include/mvicp.h; tests/boundref.py is its numpy form and its scalar-loop form.  DESIGN.md §3.20.
//
// The neighbourhoods are the rows of one internal knn_search (self mode, the max_nn nearest, within the radius if one is given, ordered by
// (dist2, original index)); a row is at most 64 long, one wave64.  One pass behind it, on the context's stream:
//   boundary   one wave per point, lane t = entry t of the row, the shape of normals_pca / normals_jet.  The lane gathers p_j and forms the
//              offset d = p_j - p_i (normals_pca.h's row_offset); the point's normal is loaded uniformly and the tangent frame (u, v) of
//              mvicp_fit_normals is formed in every lane alike; the lane projects its offset and keeps the unit direction (ex, ey) and its
//              validity.  Then a loop over the valid entries s of the row -- the ballot of the valid lanes, wave-uniform -- in which lane s's
//              direction comes by readlane (no LDS) and every lane ORs "s lies in my sector" into a flag: 2 multiplications and an
//              addition or subtraction per test, 6 fp64 operations per ordered pair.  open = the popcount of the ballot of the valid lanes
//              without a hit.  Lane 0 stores the flag byte, lanes 1 .. 3 store open, valid and used.
//   boundary_count  the number of flagged points: a strided sum of the flag bytes, one integer atomic per workgroup.
// Only comparisons, a per-lane OR and a count cross lanes, so the order the threads run in cannot show in the result.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
//
// mvicp_boundary_select: select_rows (row_select.h) over the flag bytes, one host wait for the number kept.
#include <algorithm>
#include <cstring>

#include "common.h"
#include "normals_pca.h"
#include "row_select.h"

namespace mvicp {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kThreads = 256;
constexpr int kCountBlocks = 1024;

// the control block at the start of the arena; the host reads it back through the pinned copy
struct BdCtl {
  int flagged;   // points with flag = 1 (integer atomics: exact in any order)
};

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
// lane `src`'s value (src wave-uniform) in every lane
__device__ __forceinline__ double lane_value(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void boundary_kernel(const double* __restrict__ pts, const double* __restrict__ nor, int n, int k,
                                                                       const int* __restrict__ cnt, const int* __restrict__ idx, double cos_gap,
                                                                       unsigned char* __restrict__ flag, int* __restrict__ open, int* __restrict__ valid,
                                                                       int* __restrict__ used) {
  // (one wave per point: saying so lets the point's own loads be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];   // <= k <= 64
  const double* pi = pts + 3 * (size_t)i;
  const double* Ni = nor + 3 * (size_t)i;
  const double px = pi[0], py = pi[1], pz = pi[2];
  const double N0 = Ni[0], N1 = Ni[1], N2 = Ni[2];
  const double l = __dsqrt_rn(dot3(N0, N1, N2, N0, N1, N2));
  int n_open = 0, n_valid = 0;
  if (l > 0.0 && l < __builtin_huge_val() && len >= 3) {   // (wave-uniform; a NaN fails the first comparison)
    double d0, d1, d2;
    pca::row_offset(pts, idx, i, k, len, lane, px, py, pz, d0, d1, d2);
    const double nx = __ddiv_rn(N0, l), ny = __ddiv_rn(N1, l), nz = __ddiv_rn(N2, l);
    // the tangent frame from n alone: w = e_a x n for the axis a of the smallest |n_a|, the first of equals
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const bool s1 = ay < ax;
    const bool s2 = az < (s1 ? ay : ax);
    const double w0 = s2 ? -ny : s1 ? nz : 0.0, w1 = s2 ? nx : s1 ? 0.0 : -nz, w2 = s2 ? 0.0 : s1 ? -nx : ny;
    const double lw = __dsqrt_rn(dot3(w0, w1, w2, w0, w1, w2));
    const double u0 = __ddiv_rn(w0, lw), u1 = __ddiv_rn(w1, lw), u2 = __ddiv_rn(w2, lw);
    const double v0 = __dsub_rn(__dmul_rn(ny, u2), __dmul_rn(nz, u1)), v1 = __dsub_rn(__dmul_rn(nz, u0), __dmul_rn(nx, u2)),
                 v2 = __dsub_rn(__dmul_rn(nx, u1), __dmul_rn(ny, u0));
    const double x = dot3(d0, d1, d2, u0, u1, u2), y = dot3(d0, d1, d2, v0, v1, v2);
    const double r = __dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
    const bool ok = lane < len && r > 0.0 && r < __builtin_huge_val();
    const double ex = __ddiv_rn(x, r), ey = __ddiv_rn(y, r);
    const unsigned long long vmask = __ballot(ok);
    bool hit = false;
    for (unsigned long long m = vmask; m; m &= m - 1) {   // (wave-uniform: the valid entries s in ascending order)
      const int s = __builtin_ctzll(m);
      const double sx = lane_value(ex, s), sy = lane_value(ey, s);
      const double cr = __dsub_rn(__dmul_rn(ex, sy), __dmul_rn(ey, sx));
      const double dt = __dadd_rn(__dmul_rn(ex, sx), __dmul_rn(ey, sy));
      hit = hit || (cr > 0.0 && dt > cos_gap);
    }
    n_open = __popcll(__ballot(ok && !hit));
    n_valid = __popcll(vmask);
  }
  if (lane == 0) flag[i] = n_open > 0 ? 1 : 0;
  if (lane == 1) open[i] = n_open;
  if (lane == 2) valid[i] = n_valid;
  if (lane == 3) used[i] = len;
}

// the number of flagged points: at most kCountBlocks workgroups whose lanes stride through the flag bytes, one integer atomic per workgroup
// (atomics on one address are served one after the other: their number is bounded by the grid, not by the cloud)
__global__ __launch_bounds__(kThreads) void boundary_count_kernel(const unsigned char* __restrict__ flag, int n, BdCtl* __restrict__ ctl) {
  __shared__ int s_cnt[kThreads / 64];
  int cnt = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) cnt += flag[i];
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) cnt += __shfl_xor(cnt, x, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) cnt += s_cnt[w];
    if (cnt) atomicAdd(&ctl->flagged, cnt);
  }
}

}  // namespace

long long boundary_points(mvicp_ctx* c, const FrameDev& f, int frame, const double* N, int max_nn, double radius, double B2, double cos_gap) {
  BoundaryStage& S = c->bnd;
  S.drop_result();   // (the last result ends here; a failed call leaves none behind)
  const long long total = knn_search(c, f, nullptr, 0, 0, max_nn, radius, B2);
  if (total < 0) return total;
  const int n = f.n;
  if (n == 0) { S.n = 0; S.frame = frame; return 0; }
  hipStream_t st = c->stream;
  const size_t NN = (size_t)n;
  // one arena: [control | flag bytes | open | valid | used]
  const size_t o_flags = 256, o_open = o_flags + align256(NN), o_valid = o_open + align256(4 * NN), o_used = o_valid + align256(4 * NN);
  MV_CHECK(S.dev.reserve(o_used + align256(4 * NN)));
  MV_CHECK(S.pin.reserve(256));
  MV_CHECK(S.sel.reserve(n, false, st));   // (so that a selection allocates nothing)
  char* D = S.dev.p;
  BdCtl* d_ctl = reinterpret_cast<BdCtl*>(D);
  BdCtl* h_ctl = reinterpret_cast<BdCtl*>(S.pin.p);
  S.flag = reinterpret_cast<unsigned char*>(D + o_flags);
  S.open = reinterpret_cast<int*>(D + o_open); S.valid = reinterpret_cast<int*>(D + o_valid); S.used = reinterpret_cast<int*>(D + o_used);
  MV_HIP(hipMemsetAsync(d_ctl, 0, sizeof(BdCtl), st));
  {
    // per point its position, normal, count and index row, the 13 bytes it writes; per neighbour a position (the count pass's n bytes are not counted)
    ProfScope ps(c, "boundary", (48.0 + 4.0 + 4.0 * max_nn + 13.0) * n + 24.0 * total);
    hipLaunchKernelGGL(boundary_kernel, dim3((unsigned int)((NN + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, st, f.pts, N, n, max_nn,
                       c->knn.cnt, c->knn.idx, cos_gap, S.flag, S.open, S.valid, S.used);
    MV_HIP(hipGetLastError());
    hipLaunchKernelGGL(boundary_count_kernel, dim3((unsigned int)std::min<size_t>((NN + kThreads - 1) / kThreads, kCountBlocks)), dim3(kThreads), 0, st, S.flag, n, d_ctl);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(BdCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  const int flagged = h_ctl->flagged;
  if (flagged < 0 || flagged > n) { set_error("boundary: %d flagged of %d", flagged, n); return MVICP_ERR_INTERNAL; }
  S.n = n; S.frame = frame;
  return flagged;
}

long long boundary_select(mvicp_ctx* c, const FrameDev& f, int boundary) {
  return select_rows(c, c->bnd.sel, f, "boundary select", "boundary_compact", f.nor ? 109.0 : 61.0, c->bnd.flag, boundary ? 1 : 0);
}

}  // namespace mvicp
