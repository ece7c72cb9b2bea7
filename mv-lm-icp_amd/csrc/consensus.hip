// Consensus coarse pose (mvicp_consensus): H rigid hypotheses, each from three index-aligned pairs (p, q) drawn by a counter-based
// generator, each scored against every pair; the winner is the largest inlier count, the lowest h among equals.  A pure function of the
// input bytes, bit for bit.  The contract is stated in include/mvicp.h; tests/matchref.py is its numpy form and its scalar-loop form.
// DESIGN.md §3.11.
//
// The transform of a hypothesis is the one that maps the orthonormal frame of its p triangle onto the frame of its q triangle: + - x /
// sqrt only, no SVD and no eigen-solver, so nothing is rounded differently on the host and on the GPU.  fp64, every operation rounded on
// its own; comparisons are IEEE as written.
//   1  cons_hyp_kernel    one lane per hypothesis: sample, distinctness, edge check, degenerate frames; count[h] = 0 or -1 and the
//                         accepted h compacted (ballot + one atomic per wave) -- with edge_sim = 0.9 more than 90 % are rejected on real
//                         matches, and the scoring pass does not carry those lanes
//   2  cons_score_kernel  lane = accepted hypothesis, (R, t) rebuilt from h into registers (the same device function: the same bits); the
//                         pairs staged in LDS tiles and broadcast to all lanes; an integer count per lane; the pairs split over blockIdx.y
//                         with an integer atomicAdd into count[h] when the hypotheses are few.  Integer counts make every order exact.
//   3  cons_pick_kernel   max over the keys (count + 1) << 32 | (2^32 - 1 - h): the largest count, the lowest h
//      cons_flags_kernel  the winner's pose once more, its inlier flags, the result record
#include "common.h"
#include "cons_pose.h"

namespace mvicp {

namespace {

using namespace cons_pose;
constexpr int kThreads = 256;
constexpr int kPairTile = 256;    // pairs per LDS tile of the scoring pass
constexpr int kWantBlocks = 1024; // the scoring pass splits the pairs until it has about this many workgroups

struct ConsCtl { int n_acc; int nonfinite; unsigned long long key; mvicp_consensus_result res; };

__global__ __launch_bounds__(kThreads) void cons_hyp_kernel(const double* __restrict__ P, const double* __restrict__ Q, int c, int H,
                                                            unsigned long long seed, double s2, int* __restrict__ count, int* __restrict__ hidx,
                                                            ConsCtl* __restrict__ ctl) {
  const int h = (int)(blockIdx.x * kThreads + threadIdx.x), lane = threadIdx.x & 63;   // (H <= 2^24)
  const bool ok = h < H && hypothesis<false>(P, Q, (unsigned long long)c, seed, (unsigned int)h, s2, nullptr, nullptr);
  if (h < H) count[h] = ok ? 0 : -1;
  const unsigned long long mask = __ballot(ok);
  if (mask == 0ull) return;
  const int first = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(&ctl->n_acc, __popcll(mask));
  base = __shfl(base, first);
  if (ok) hidx[base + __popcll(mask & ((1ull << lane) - 1ull))] = h;
}

__global__ __launch_bounds__(kThreads) void cons_score_kernel(const double* __restrict__ P, const double* __restrict__ Q, int c, unsigned long long seed,
                                                              double s2, double tau2, const int* __restrict__ hidx, int n_acc, int per_y,
                                                              int* __restrict__ count) {
  __shared__ double Sp[3 * kPairTile];
  __shared__ double Sq[3 * kPairTile];
  const int slot = (int)(blockIdx.x * kThreads + threadIdx.x);
  bool live = slot < n_acc;
  const int h = live ? hidx[slot] : 0;
  double R[9], t[3];
  if (live) live = hypothesis<true>(P, Q, (unsigned long long)c, seed, (unsigned int)h, s2, R, t);   // (always accepted: pass 1 decided with the same code)
  if (!live) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
  }
  const long long lo = (long long)blockIdx.y * per_y;
  const long long hi = lo + per_y < (long long)c ? lo + per_y : (long long)c;
  int cnt = 0;
  for (long long base = lo; base < hi; base += kPairTile) {
    const int rows = (int)(hi - base < kPairTile ? hi - base : kPairTile);
    __syncthreads();   // (the last tile has been read by every wave)
    for (int e = threadIdx.x; e < 3 * rows; e += kThreads) { Sp[e] = P[3 * (size_t)base + e]; Sq[e] = Q[3 * (size_t)base + e]; }
    __syncthreads();
    for (int r = 0; r < rows; ++r) cnt += inlier(R, t, Sp + 3 * r, Sq + 3 * r, tau2) ? 1 : 0;
  }
  if (live && cnt) atomicAdd(&count[h], cnt);
}

__global__ __launch_bounds__(kThreads) void cons_pick_kernel(const int* __restrict__ count, int H, ConsCtl* __restrict__ ctl) {
  const int h = (int)(blockIdx.x * kThreads + threadIdx.x);
  const int n = h < H ? count[h] : -1;
  unsigned long long key = n >= 0 ? ((unsigned long long)((unsigned int)n + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)h) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&ctl->key, key);
}

__global__ __launch_bounds__(kThreads) void cons_flags_kernel(const double* __restrict__ P, const double* __restrict__ Q, int c, unsigned long long seed,
                                                              double s2, double tau2, unsigned char* __restrict__ flags, ConsCtl* __restrict__ ctl) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long key = ctl->key;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  int best = -1, n = 0;
  if (key) {
    best = (int)(0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull));
    n = (int)(key >> 32) - 1;
    (void)hypothesis<true>(P, Q, (unsigned long long)c, seed, (unsigned int)best, s2, R, t);
  }
  if (i < c) flags[i] = key && inlier(R, t, P + 3 * i, Q + 3 * i, tau2) ? 1 : 0;
  if (i == 0) {
    mvicp_consensus_result* o = &ctl->res;
    o->best = best; o->count = n; o->accepted = ctl->n_acc; o->reserved = 0;
#pragma unroll
    for (int col = 0; col < 3; ++col) {   // column-major 4 x 4
#pragma unroll
      for (int r = 0; r < 3; ++r) o->pose[4 * col + r] = R[3 * r + col];
      o->pose[4 * col + 3] = 0.0;
    }
    o->pose[12] = t[0]; o->pose[13] = t[1]; o->pose[14] = t[2]; o->pose[15] = 1.0;
  }
}

__global__ __launch_bounds__(kThreads) void cons_finite_kernel(const double* __restrict__ v, size_t count, int* __restrict__ flag) {
  bool bad = false;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < count; e += (size_t)gridDim.x * kThreads) bad |= !isfinite(v[e]);
  if (bad) atomicOr(flag, 1);
}

}  // namespace

int consensus(mvicp_ctx* c, const double* P, int p_on_device, const double* Q, int q_on_device, long long n_pairs, long long H, unsigned long long seed,
              double tau, double edge_sim, mvicp_consensus_result* out) {
  c->cons.H = -1; c->cons.c = -1;   // (the last result ends here; a failed call leaves none behind)
  hipStream_t st = c->stream;
  const size_t C = (size_t)n_pairs, NH = (size_t)H;
  // [ctl | count H | accepted h | flags c | P staged | Q staged]
  const size_t off_count = 256, off_hidx = off_count + align256(4 * NH), off_flags = off_hidx + align256(4 * NH), off_p = off_flags + align256(C);
  const size_t off_q = off_p + (p_on_device ? 0 : align256(24 * C)), need = off_q + (q_on_device ? 0 : align256(24 * C));
  static_assert(sizeof(ConsCtl) <= 256, "the control record fits its slot");
  MV_CHECK(c->cons.dev.reserve(need));
  ConsCtl* ctl = reinterpret_cast<ConsCtl*>(c->cons.dev.p);
  c->cons.count = reinterpret_cast<int*>(c->cons.dev.p + off_count);
  int* hidx = reinterpret_cast<int*>(c->cons.dev.p + off_hidx);
  c->cons.flags = reinterpret_cast<unsigned char*>(c->cons.dev.p + off_flags);
  const double* dP = P; const double* dQ = Q;
  if (!p_on_device) { MV_HIP(hipMemcpyAsync(c->cons.dev.p + off_p, P, 24 * C, hipMemcpyHostToDevice, st)); dP = reinterpret_cast<const double*>(c->cons.dev.p + off_p); }
  if (!q_on_device) { MV_HIP(hipMemcpyAsync(c->cons.dev.p + off_q, Q, 24 * C, hipMemcpyHostToDevice, st)); dQ = reinterpret_cast<const double*>(c->cons.dev.p + off_q); }
  MV_HIP(hipMemsetAsync(ctl, 0, sizeof(ConsCtl), st));
  const size_t wgs_c = (3 * C + kThreads - 1) / kThreads;
  const dim3 grid_fin((unsigned int)(wgs_c < 4096 ? wgs_c : 4096));
  hipLaunchKernelGGL(cons_finite_kernel, grid_fin, dim3(kThreads), 0, st, dP, 3 * C, &ctl->nonfinite);
  hipLaunchKernelGGL(cons_finite_kernel, grid_fin, dim3(kThreads), 0, st, dQ, 3 * C, &ctl->nonfinite);
  MV_HIP(hipGetLastError());
  ConsCtl h_ctl;
  MV_HIP(hipMemcpyAsync(&h_ctl, ctl, sizeof(ConsCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (h_ctl.nonfinite) { set_error("a coordinate is not finite"); return MVICP_ERR_ARG; }
  const double s2 = edge_sim * edge_sim, tau2 = tau * tau;
  const dim3 block(kThreads), grid_h((unsigned int)((NH + kThreads - 1) / kThreads));
  {
    ProfScope ps(c, "cons_hyp", 8.0 * NH + 144.0 * NH);   // count and the accepted list; six points per hypothesis
    hipLaunchKernelGGL(cons_hyp_kernel, grid_h, block, 0, st, dP, dQ, (int)n_pairs, (int)H, seed, s2, c->cons.count, hidx, ctl);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(&h_ctl, ctl, sizeof(ConsCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  const int n_acc = h_ctl.n_acc;
  if (n_acc > 0) {
    const int gx = (n_acc + kThreads - 1) / kThreads;
    const long long tiles = ((long long)n_pairs + kPairTile - 1) / kPairTile;
    long long gy = (kWantBlocks + gx - 1) / gx;
    if (gy > tiles) gy = tiles;
    if (gy > 65535) gy = 65535;
    if (gy < 1) gy = 1;
    const long long per_y = ((tiles + gy - 1) / gy) * kPairTile;   // (whole tiles: < 2^31 + 256 fits an int only below 2^31, see the clamp)
    const int per_y_i = (int)(per_y < (long long)n_pairs ? per_y : (long long)n_pairs);
    const unsigned int gy_u = (unsigned int)(((long long)n_pairs + per_y_i - 1) / per_y_i);
    ProfScope ps(c, "cons_score", (48.0 * C) * gx + 148.0 * n_acc);   // every workgroup column reads every pair once
    hipLaunchKernelGGL(cons_score_kernel, dim3((unsigned int)gx, gy_u), block, 0, st, dP, dQ, (int)n_pairs, seed, s2, tau2, hidx, n_acc, per_y_i, c->cons.count);
    MV_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "cons_pick", 4.0 * NH + 49.0 * C);
    hipLaunchKernelGGL(cons_pick_kernel, grid_h, block, 0, st, c->cons.count, (int)H, ctl);
    hipLaunchKernelGGL(cons_flags_kernel, dim3((unsigned int)((C + kThreads - 1) / kThreads)), block, 0, st, dP, dQ, (int)n_pairs, seed, s2, tau2, c->cons.flags, ctl);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(&h_ctl, ctl, sizeof(ConsCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (out) *out = h_ctl.res;
  c->cons.H = H; c->cons.c = n_pairs;
  return MVICP_OK;
}

}  // namespace mvicp
