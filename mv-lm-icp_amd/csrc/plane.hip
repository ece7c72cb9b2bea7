// RANSAC plane segmentation over one stored cloud (mvicp_segment_plane, mvicp_plane_select): H plane hypotheses, each from three points
// drawn by the counter-based generator of the consensus stage, each scored against every point; the winner is the largest inlier count,
// the lowest h among equals; its inliers are refitted through exact integer moments.  A pure function of the stored bytes and the
// arguments, bit for bit (the contract is stated in include/mvicp.h; tests/planeref.py is its numpy form and its scalar-loop form).
// Only comparisons, integer sums and a maximum cross lanes, so no order of the threads can change a bit.  DESIGN.md §3.19.
//
// Passes of mvicp_segment_plane, all on the context's stream:
//   1  plane_hyp_kernel      one lane per hypothesis: sample, distinctness, the unit normal, the direction test; count[h] = 0 or -1 and
//                            the accepted h compacted (ballot + one atomic per wave), as cons_hyp_kernel does
//   2  plane_score_kernel    lane = accepted hypothesis, (a, m) rebuilt from h into registers by the same device function (the same bits);
//                            the points staged in LDS tiles and read as a broadcast; an int count per lane; the points split over
//                            blockIdx.y with one integer atomicAdd per lane and chunk.  The number accepted is read from the control block
//                            on the device: the host does not wait for it, and workgroups past it return at once.
//   3  plane_pick_kernel     max over the keys (count + 1) << 32 | (2^32 - 1 - h): the largest count, the lowest h
//   4  plane_flags_kernel    the winner once more: its inlier flags and omax, the largest |offset| over them (a maximum of non-negative
//                            doubles is an integer maximum of their bits: per lane over its points, wave reduction, LDS across the waves,
//                            one atomicMax per workgroup)
//   5  plane_moments_kernel  (refine) b and q from the winner's count and omax, M = floor(ldexp(o, q)); the count and the nine sums of M and
//                            M M^T as int64: per lane over its points, wave reduction, LDS across the waves, ten 64-bit integer atomics
//                            per workgroup
//      -- host wait: the control block; the host rule mvicp_plane_from_moments gives the refined plane --
//   6  plane_final_kernel    (refit) the flags by the refined plane and their number (one integer atomic per workgroup)
//      Passes 4 to 6 run at most kStreamBlocks workgroups whose lanes stride through the cloud: atomics on one address are served one
//      after the other, so their number is bounded by the grid and not by the cloud.
//      -- host wait: the number of refined inliers --
// mvicp_plane_select: select_rows (row_select.h) over the flag bytes, one host wait for the number kept.
// Every store is a plain vector store or a vector atomic; no kernel waits for another workgroup.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "cons_pose.h"
#include "row_select.h"

namespace mvicp {

namespace {

using cons_pose::cross1;
using cons_pose::dot3;
using cons_pose::sample_index;

constexpr int kThreads = 256;      // lanes per workgroup of every kernel here
constexpr int kPointTile = 256;    // points per LDS tile of the scoring pass
constexpr int kWantBlocks = 1024;  // the scoring pass splits the points until it has about this many workgroups
// the passes over the points run at most this many workgroups, each lane striding through the cloud: one atomic per workgroup and result
// word (atomics on one address are served one after the other, so their number must not grow with the cloud)
constexpr int kStreamBlocks = 1024;

// the direction test: on = 0 without an axis; rhs = (cos_min * cos_min) * dot(axis, axis), formed once on the host
struct PlDir { int on, pad; double ax, ay, az, rhs; };

struct PlCtl {
  int n_acc, final_count, b, q, pad[2];
  unsigned long long key;    // the winner's (count + 1) << 32 | (2^32 - 1 - h); 0: nothing accepted
  unsigned long long omax;   // bit pattern of the largest |offset| over the winner's inliers
  long long mom[10];         // c, s0 s1 s2, S00 S01 S02 S11 S12 S22
  double a[3], m[3];         // the winning hypothesis
};
static_assert(sizeof(PlCtl) <= 256, "the control record fits its slot");

// hypothesis h: accepted?  With WANT also a (the first sample) and m (the unit normal)
template <bool WANT>
__device__ __forceinline__ bool plane_hypothesis(const double* __restrict__ P, unsigned long long n, unsigned long long seed, unsigned int h, const PlDir& dir,
                                                 double* a, double* m) {
  const unsigned long long i0 = sample_index(seed, h, 0, n), i1 = sample_index(seed, h, 1, n), i2 = sample_index(seed, h, 2, n);
  if (i0 == i1 || i1 == i2 || i2 == i0) return false;   // (before every load: n < 3 ends here)
  const double a0 = P[3 * i0], a1 = P[3 * i0 + 1], a2 = P[3 * i0 + 2];
  const double ux = __dsub_rn(P[3 * i1], a0), uy = __dsub_rn(P[3 * i1 + 1], a1), uz = __dsub_rn(P[3 * i1 + 2], a2);
  const double vx = __dsub_rn(P[3 * i2], a0), vy = __dsub_rn(P[3 * i2 + 1], a1), vz = __dsub_rn(P[3 * i2 + 2], a2);
  const double wx = cross1(uy, uz, vy, vz), wy = cross1(uz, ux, vz, vx), wz = cross1(ux, uy, vx, vy);
  const double nw = __dsqrt_rn(dot3(wx, wy, wz, wx, wy, wz));
  if (!(nw > 0.0 && nw < INFINITY)) return false;
  const double mx = __ddiv_rn(wx, nw), my = __ddiv_rn(wy, nw), mz = __ddiv_rn(wz, nw);
  if (dir.on) {
    const double da = dot3(mx, my, mz, dir.ax, dir.ay, dir.az);
    if (!(__dmul_rn(da, da) >= dir.rhs)) return false;
  }
  if (WANT) { a[0] = a0; a[1] = a1; a[2] = a2; m[0] = mx; m[1] = my; m[2] = mz; }
  return true;
}

// r = dot(m, p - g): the offset first, then the dot product
__device__ __forceinline__ double residual(const double* m, const double* g, double px, double py, double pz) {
  return dot3(m[0], m[1], m[2], __dsub_rn(px, g[0]), __dsub_rn(py, g[1]), __dsub_rn(pz, g[2]));
}

__global__ __launch_bounds__(kThreads) void plane_hyp_kernel(const double* __restrict__ P, int n, int H, unsigned long long seed, PlDir dir, int* __restrict__ count,
                                                             int* __restrict__ hidx, PlCtl* __restrict__ ctl) {
  const int h = (int)(blockIdx.x * kThreads + threadIdx.x), lane = threadIdx.x & 63;   // (H <= 2^24)
  const bool ok = h < H && plane_hypothesis<false>(P, (unsigned long long)n, seed, (unsigned int)h, dir, nullptr, nullptr);
  if (h < H) count[h] = ok ? 0 : -1;
  const unsigned long long mask = __ballot(ok);
  if (mask == 0ull) return;
  const int first = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(&ctl->n_acc, __popcll(mask));
  base = __shfl(base, first);
  if (ok) hidx[base + __popcll(mask & ((1ull << lane) - 1ull))] = h;   // (base + rank < the number accepted <= H)
}

__global__ __launch_bounds__(kThreads) void plane_score_kernel(const double* __restrict__ P, int n, unsigned long long seed, PlDir dir, double tau,
                                                               const int* __restrict__ hidx, const PlCtl* __restrict__ ctl, int per_y, int* __restrict__ count) {
  __shared__ double Sp[3 * kPointTile];
  const int n_acc = ctl->n_acc;   // (complete: written by the kernel before this one)
  if ((int)(blockIdx.x * kThreads) >= n_acc) return;   // (the whole workgroup: the grid is sized for H, not for the number accepted)
  const int slot = (int)(blockIdx.x * kThreads + threadIdx.x);
  bool live = slot < n_acc;
  const int h = live ? hidx[slot] : 0;
  double a[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
  if (live) live = plane_hypothesis<true>(P, (unsigned long long)n, seed, (unsigned int)h, dir, a, m);   // (always accepted: pass 1 decided with the same code)
  const long long lo = (long long)blockIdx.y * per_y;
  const long long hi = lo + per_y < (long long)n ? lo + per_y : (long long)n;
  int cnt = 0;
  for (long long base = lo; base < hi; base += kPointTile) {
    const int rows = (int)(hi - base < kPointTile ? hi - base : kPointTile);
    __syncthreads();   // (the last tile has been read by every wave)
    for (int e = threadIdx.x; e < 3 * rows; e += kThreads) Sp[e] = P[3 * (size_t)base + e];   // (base + rows <= hi <= n)
    __syncthreads();
    for (int r = 0; r < rows; ++r) cnt += fabs(residual(m, a, Sp[3 * r], Sp[3 * r + 1], Sp[3 * r + 2])) <= tau ? 1 : 0;
  }
  if (live && cnt) atomicAdd(&count[h], cnt);
}

__global__ __launch_bounds__(kThreads) void plane_pick_kernel(const int* __restrict__ count, int H, PlCtl* __restrict__ ctl) {
  const int h = (int)(blockIdx.x * kThreads + threadIdx.x);
  const int c = h < H ? count[h] : -1;
  unsigned long long key = c >= 0 ? ((unsigned long long)((unsigned int)c + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)h) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&ctl->key, key);
}

__global__ __launch_bounds__(kThreads) void plane_flags_kernel(const double* __restrict__ P, int n, unsigned long long seed, PlDir dir, double tau,
                                                               unsigned char* __restrict__ flags, PlCtl* __restrict__ ctl) {
  __shared__ unsigned long long s_max[kThreads / 64];
  const unsigned long long key = ctl->key;   // (complete: written by the kernel before this one; this kernel writes omax, a and m only)
  double a[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
  if (key) (void)plane_hypothesis<true>(P, (unsigned long long)n, seed, 0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull), dir, a, m);
  double om = 0.0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    bool in = false;
    if (key) {
      const double px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
      in = fabs(residual(m, a, px, py, pz)) <= tau;
      if (in) om = fmax(om, fmax(fmax(fabs(__dsub_rn(px, a[0])), fabs(__dsub_rn(py, a[1]))), fabs(__dsub_rn(pz, a[2]))));   // (finite: the residual is)
    }
    flags[i] = in ? 1 : 0;
  }
  unsigned long long bits = (unsigned long long)__double_as_longlong(om);   // om >= +0: the bit patterns order like the values
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { const unsigned long long o = __shfl_xor(bits, x, 64); bits = o > bits ? o : bits; }
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) bits = s_max[w] > bits ? s_max[w] : bits;
    if (bits != 0ull) atomicMax(&ctl->omax, bits);
    if (blockIdx.x == 0 && key) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { ctl->a[k] = a[k]; ctl->m[k] = m[k]; }
    }
  }
}

// the bit budget of c inliers and the scale exponent of omax > 0: 2^(b-1) <= omax 2^q < 2^b
__host__ __device__ __forceinline__ void bit_rule(int c, double omax, int* b, int* q) {
  int L = 0;
  for (unsigned int v = (unsigned int)c; v; v >>= 1) ++L;
  const int bb = (62 - L) / 2 < 21 ? (62 - L) / 2 : 21;
  int ex = 0;
  (void)frexp(omax, &ex);   // omax = f 2^ex, f in [0.5, 1)
  *b = bb; *q = bb - ex;
}

__global__ __launch_bounds__(kThreads) void plane_moments_kernel(const double* __restrict__ P, int n, const unsigned char* __restrict__ flags, PlCtl* __restrict__ ctl) {
  __shared__ long long s_p[kThreads / 64][10];
  const unsigned long long key = ctl->key, obits = ctl->omax;   // (complete: written by the kernels before this one)
  if (!key || !obits) return;   // (the whole grid: no winner, or every inlier is the point a itself -- the refit is refused)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b, q;
  bit_rule((int)(key >> 32) - 1, __longlong_as_double((long long)obits), &b, &q);
  const double a0 = ctl->a[0], a1 = ctl->a[1], a2 = ctl->a[2];
  long long v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (a lane's share of sums that fit int64 as a whole)
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    if (!flags[i]) continue;
    const long long M0 = (long long)floor(ldexp(__dsub_rn(P[3 * i], a0), q));       // |M| <= 2^b <= 2^21
    const long long M1 = (long long)floor(ldexp(__dsub_rn(P[3 * i + 1], a1), q));
    const long long M2 = (long long)floor(ldexp(__dsub_rn(P[3 * i + 2], a2), q));
    v[0] += 1; v[1] += M0; v[2] += M1; v[3] += M2;
    v[4] += M0 * M0; v[5] += M0 * M1; v[6] += M0 * M2; v[7] += M1 * M1; v[8] += M1 * M2; v[9] += M2 * M2;
  }
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) v[t] += __shfl_xor(v[t], x, 64);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < 10; ++t) s_p[wave][t] = v[t];
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    const int t = threadIdx.x;
    long long sum = s_p[0][t];
    for (int w = 1; w < kThreads / 64; ++w) sum += s_p[w][t];
    if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(&ctl->mom[t]), (unsigned long long)sum);   // (two's complement: the sum of the parts)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->b = b; ctl->q = q; }
}

struct PlPlane { double m[3], g[3]; };

__global__ __launch_bounds__(kThreads) void plane_final_kernel(const double* __restrict__ P, int n, PlPlane pl, double tau, unsigned char* __restrict__ flags,
                                                               PlCtl* __restrict__ ctl) {
  __shared__ int s_cnt[kThreads / 64];
  int cnt = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const bool in = fabs(residual(pl.m, pl.g, P[3 * i], P[3 * i + 1], P[3 * i + 2])) <= tau;
    flags[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) cnt += __shfl_xor(cnt, x, 64);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) cnt += s_cnt[w];
    if (cnt) atomicAdd(&ctl->final_count, cnt);
  }
}

double plane_d(const double* m, const double* g) { return -((m[0] * g[0] + m[1] * g[1]) + m[2] * g[2]); }   // (this file is built without fma contraction)

}  // namespace

int plane_segment(mvicp_ctx* c, const FrameDev& f, int frame, long long H, unsigned long long seed, double tau, const double* axis, double cos_min, int refine,
                  mvicp_plane_result* out) {
  PlaneStage& S = c->plane;
  S.drop_result();   // (the last result ends here; a failed call leaves none behind)
  mvicp_plane_result R;
  std::memset(&R, 0, sizeof(R));
  R.best = -1; R.n = f.n; R.has_normals = f.nor ? 1 : 0;
  const int n = f.n;
  const size_t NN = (size_t)n, NH = (size_t)H;
  hipStream_t st = c->stream;

  // one arena: [control | count | accepted h | flags]
  const size_t o_count = 256, o_hidx = o_count + align256(4 * NH), o_flags = o_hidx + align256(4 * NH);
  MV_CHECK(S.dev.reserve(o_flags + align256(std::max<size_t>(NN, 1))));
  MV_CHECK(S.pin.reserve(256));
  if (n > 0) MV_CHECK(S.sel.reserve(n, false, st));   // (so that a selection allocates nothing)
  char* D = S.dev.p;
  PlCtl* d_ctl = reinterpret_cast<PlCtl*>(D);
  PlCtl* h_ctl = reinterpret_cast<PlCtl*>(S.pin.p);
  S.count = reinterpret_cast<int*>(D + o_count); S.flags = reinterpret_cast<unsigned char*>(D + o_flags);
  int* hidx = reinterpret_cast<int*>(D + o_hidx);

  PlDir dir;
  std::memset(&dir, 0, sizeof(dir));
  if (axis) {
    dir.on = 1; dir.ax = axis[0]; dir.ay = axis[1]; dir.az = axis[2];
    dir.rhs = (cos_min * cos_min) * ((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
  }
  MV_HIP(hipMemsetAsync(d_ctl, 0, sizeof(PlCtl), st));
  const dim3 block(kThreads), grid_h((unsigned int)((NH + kThreads - 1) / kThreads)), grid_n((unsigned int)std::min<size_t>((NN + kThreads - 1) / kThreads, kStreamBlocks));
  {
    ProfScope ps(c, "plane_hyp", 8.0 * NH + 72.0 * NH);   // count and the accepted list; three points per hypothesis
    hipLaunchKernelGGL(plane_hyp_kernel, grid_h, block, 0, st, f.pts, n, (int)H, seed, dir, S.count, hidx, d_ctl);
  }
  MV_HIP(hipGetLastError());
  if (n > 0) {
    // the grid covers every hypothesis (the number accepted stays on the device); the points are split until the device is full
    const long long gx = (long long)grid_h.x;
    const long long tiles = ((long long)n + kPointTile - 1) / kPointTile;
    long long gy = (kWantBlocks + gx - 1) / gx;
    if (gy > tiles) gy = tiles;
    if (gy > 65535) gy = 65535;
    if (gy < 1) gy = 1;
    const long long per_y = ((tiles + gy - 1) / gy) * kPointTile;   // whole tiles
    const int per_y_i = (int)(per_y < (long long)n ? per_y : (long long)n);
    const unsigned int gy_u = (unsigned int)(((long long)n + per_y_i - 1) / per_y_i);
    {
      ProfScope ps(c, "plane_score", (24.0 * NN) * (double)gx + 76.0 * NH);   // every workgroup column reads every point once
      hipLaunchKernelGGL(plane_score_kernel, dim3((unsigned int)gx, gy_u), block, 0, st, f.pts, n, seed, dir, tau, hidx, d_ctl, per_y_i, S.count);
    }
    MV_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "plane_pick", 4.0 * NH);
    hipLaunchKernelGGL(plane_pick_kernel, grid_h, block, 0, st, S.count, (int)H, d_ctl);
  }
  MV_HIP(hipGetLastError());
  if (n > 0) {
    {
      ProfScope ps(c, "plane_flags", 25.0 * NN);
      hipLaunchKernelGGL(plane_flags_kernel, grid_n, block, 0, st, f.pts, n, seed, dir, tau, S.flags, d_ctl);
    }
    MV_HIP(hipGetLastError());
    if (refine) {
      ProfScope ps(c, "plane_moments", 25.0 * NN);
      hipLaunchKernelGGL(plane_moments_kernel, grid_n, block, 0, st, f.pts, n, S.flags, d_ctl);
    }
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(PlCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  R.accepted = h_ctl->n_acc;
  if (h_ctl->n_acc < 0 || h_ctl->n_acc > H || (h_ctl->key != 0) != (h_ctl->n_acc > 0 && n > 0)) {
    set_error("plane: %d of %lld hypotheses accepted, key %llx", h_ctl->n_acc, H, h_ctl->key);
    return MVICP_ERR_INTERNAL;
  }
  if (h_ctl->key) {
    R.best = (int)(0xFFFFFFFFu - (unsigned int)(h_ctl->key & 0xFFFFFFFFull));
    R.count = (int)(h_ctl->key >> 32) - 1;
    R.count_refined = R.count;
    for (int k = 0; k < 3; ++k) { R.hyp_normal[k] = R.normal[k] = h_ctl->m[k]; R.hyp_point[k] = R.point[k] = h_ctl->a[k]; }
    double omax;
    std::memcpy(&omax, &h_ctl->omax, 8);
    if (refine && omax > 0.0) {
      int b, q;
      bit_rule(R.count, omax, &b, &q);
      if (b != h_ctl->b || q != h_ctl->q || h_ctl->mom[0] != R.count) {
        set_error("plane: the device's refit used b %d q %d over %lld inliers, the host rule gives b %d q %d over %d", h_ctl->b, h_ctl->q, h_ctl->mom[0], b, q, R.count);
        return MVICP_ERR_INTERNAL;
      }
      PlPlane pl;
      MV_CHECK(mvicp_plane_from_moments(R.count, h_ctl->mom + 1, h_ctl->mom + 4, q, h_ctl->a, h_ctl->m, pl.m, pl.g));
      {
        ProfScope ps(c, "plane_flags", 25.0 * NN);
        hipLaunchKernelGGL(plane_final_kernel, grid_n, block, 0, st, f.pts, n, pl, tau, S.flags, d_ctl);
      }
      MV_HIP(hipGetLastError());
      MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(PlCtl), hipMemcpyDeviceToHost, st));
      MV_HIP(hipStreamSynchronize(st));
      if (h_ctl->final_count < 0 || h_ctl->final_count > n) { set_error("plane: %d refined inliers of %d", h_ctl->final_count, n); return MVICP_ERR_INTERNAL; }
      R.refit = 1; R.b = b; R.q = q; R.count_refined = h_ctl->final_count;
      for (int k = 0; k < 3; ++k) { R.normal[k] = pl.m[k]; R.point[k] = pl.g[k]; }
    }
    R.d = plane_d(R.normal, R.point);
  }
  if (out) *out = R;
  S.n = n; S.H = H; S.frame = frame;
  return MVICP_OK;
}

long long plane_select(mvicp_ctx* c, const FrameDev& f, int inliers) {
  return select_rows(c, c->plane.sel, f, "plane select", "plane_compact", f.nor ? 109.0 : 61.0, c->plane.flags, inliers ? 1 : 0);
}

}  // namespace mvicp
