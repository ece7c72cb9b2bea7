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

namespace mvicp {

namespace {

constexpr int kThreads = 256;
constexpr int kPairTile = 256;    // pairs per LDS tile of the scoring pass
constexpr int kWantBlocks = 1024; // the scoring pass splits the pairs until it has about this many workgroups

struct ConsCtl { int n_acc; int nonfinite; unsigned long long key; mvicp_consensus_result res; };

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}
__device__ __forceinline__ double cross1(double a1, double a2, double b1, double b2) { return __dsub_rn(__dmul_rn(a1, b2), __dmul_rn(a2, b1)); }

__device__ __forceinline__ unsigned long long sample_index(unsigned long long seed, unsigned int h, int t, unsigned long long c) {
  unsigned long long z = seed + (3ull * h + (unsigned long long)t + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  const unsigned long long u = z ^ (z >> 31);
  return ((u >> 32) * c) >> 32;
}

// the orthonormal frame (e1, e2, e3) of the triangle T (three points, 9 doubles); false: a degenerate triangle
__device__ __forceinline__ bool tri_frame(const double* T, double* e1, double* e2, double* e3) {
  const double ux = __dsub_rn(T[3], T[0]), uy = __dsub_rn(T[4], T[1]), uz = __dsub_rn(T[5], T[2]);
  const double n1 = __dsqrt_rn(dot3(ux, uy, uz, ux, uy, uz));
  if (n1 == 0.0) return false;
  e1[0] = __ddiv_rn(ux, n1); e1[1] = __ddiv_rn(uy, n1); e1[2] = __ddiv_rn(uz, n1);
  const double vx = __dsub_rn(T[6], T[0]), vy = __dsub_rn(T[7], T[1]), vz = __dsub_rn(T[8], T[2]);
  const double wx = cross1(e1[1], e1[2], vy, vz), wy = cross1(e1[2], e1[0], vz, vx), wz = cross1(e1[0], e1[1], vx, vy);
  const double nw = __dsqrt_rn(dot3(wx, wy, wz, wx, wy, wz));
  if (nw == 0.0) return false;
  e3[0] = __ddiv_rn(wx, nw); e3[1] = __ddiv_rn(wy, nw); e3[2] = __ddiv_rn(wz, nw);
  e2[0] = cross1(e3[1], e3[2], e1[1], e1[2]); e2[1] = cross1(e3[2], e3[0], e1[2], e1[0]); e2[2] = cross1(e3[0], e3[1], e1[0], e1[1]);
  return true;
}

// hypothesis h: accepted?  With WANT_POSE also R (row-major) and t
template <bool WANT_POSE>
__device__ __forceinline__ bool hypothesis(const double* __restrict__ P, const double* __restrict__ Q, unsigned long long c, unsigned long long seed,
                                           unsigned int h, double s2, double* R, double* t) {
  const unsigned long long i0 = sample_index(seed, h, 0, c), i1 = sample_index(seed, h, 1, c), i2 = sample_index(seed, h, 2, c);
  if (i0 == i1 || i1 == i2 || i2 == i0) return false;
  double TP[9], TQ[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    TP[k] = P[3 * i0 + k]; TP[3 + k] = P[3 * i1 + k]; TP[6 + k] = P[3 * i2 + k];
    TQ[k] = Q[3 * i0 + k]; TQ[3 + k] = Q[3 * i1 + k]; TQ[6 + k] = Q[3 * i2 + k];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {   // the edges (0,1), (1,2), (2,0)
    const int a = 3 * e, b = 3 * ((e + 1) % 3);
    const double px = __dsub_rn(TP[a], TP[b]), py = __dsub_rn(TP[a + 1], TP[b + 1]), pz = __dsub_rn(TP[a + 2], TP[b + 2]);
    const double qx = __dsub_rn(TQ[a], TQ[b]), qy = __dsub_rn(TQ[a + 1], TQ[b + 1]), qz = __dsub_rn(TQ[a + 2], TQ[b + 2]);
    const double lp = dot3(px, py, pz, px, py, pz), lq = dot3(qx, qy, qz, qx, qy, qz);
    if (!(lp >= __dmul_rn(s2, lq) && lq >= __dmul_rn(s2, lp))) return false;
  }
  double e1[3], e2[3], e3[3], f1[3], f2[3], f3[3];
  if (!tri_frame(TP, e1, e2, e3) || !tri_frame(TQ, f1, f2, f3)) return false;
  if (WANT_POSE) {
    double cp[3], cq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cp[k] = __ddiv_rn(__dadd_rn(__dadd_rn(TP[k], TP[3 + k]), TP[6 + k]), 3.0);
      cq[k] = __ddiv_rn(__dadd_rn(__dadd_rn(TQ[k], TQ[3 + k]), TQ[6 + k]), 3.0);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) R[3 * r + k] = __dadd_rn(__dadd_rn(__dmul_rn(f1[r], e1[k]), __dmul_rn(f2[r], e2[k])), __dmul_rn(f3[r], e3[k]));
      t[r] = __dsub_rn(cq[r], dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], cp[0], cp[1], cp[2]));
    }
  }
  return true;
}

__device__ __forceinline__ bool inlier(const double* R, const double* t, const double* p, const double* q, double tau2) {
  const double rx = __dsub_rn(__dadd_rn(dot3(R[0], R[1], R[2], p[0], p[1], p[2]), t[0]), q[0]);
  const double ry = __dsub_rn(__dadd_rn(dot3(R[3], R[4], R[5], p[0], p[1], p[2]), t[1]), q[1]);
  const double rz = __dsub_rn(__dadd_rn(dot3(R[6], R[7], R[8], p[0], p[1], p[2]), t[2]), q[2]);
  return dot3(rx, ry, rz, rx, ry, rz) <= tau2;
}

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

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

void free_consensus(mvicp_ctx* c) {
  if (c->cons_dev) (void)hipFree(c->cons_dev);
  c->cons_dev = nullptr; c->cons_dev_bytes = 0;
  c->cons_count = nullptr; c->cons_flags = nullptr;
  c->cons_H = -1; c->cons_c = -1;
}

int consensus(mvicp_ctx* c, const double* P, int p_on_device, const double* Q, int q_on_device, long long n_pairs, long long H, unsigned long long seed,
              double tau, double edge_sim, mvicp_consensus_result* out) {
  c->cons_H = -1; c->cons_c = -1;   // (the last result ends here; a failed call leaves none behind)
  hipStream_t st = c->stream;
  const size_t C = (size_t)n_pairs, NH = (size_t)H;
  // [ctl | count H | accepted h | flags c | P staged | Q staged]
  const size_t off_count = 256, off_hidx = off_count + align256(4 * NH), off_flags = off_hidx + align256(4 * NH), off_p = off_flags + align256(C);
  const size_t off_q = off_p + (p_on_device ? 0 : align256(24 * C)), need = off_q + (q_on_device ? 0 : align256(24 * C));
  static_assert(sizeof(ConsCtl) <= 256, "the control record fits its slot");
  if (need > c->cons_dev_bytes) {
    if (c->cons_dev) MV_HIP(hipFree(c->cons_dev));
    c->cons_dev = nullptr; c->cons_dev_bytes = 0;
    MV_HIP(hipMalloc((void**)&c->cons_dev, need));
    c->cons_dev_bytes = need;
  }
  ConsCtl* ctl = reinterpret_cast<ConsCtl*>(c->cons_dev);
  c->cons_count = reinterpret_cast<int*>(c->cons_dev + off_count);
  int* hidx = reinterpret_cast<int*>(c->cons_dev + off_hidx);
  c->cons_flags = reinterpret_cast<unsigned char*>(c->cons_dev + off_flags);
  const double* dP = P; const double* dQ = Q;
  if (!p_on_device) { MV_HIP(hipMemcpyAsync(c->cons_dev + off_p, P, 24 * C, hipMemcpyHostToDevice, st)); dP = reinterpret_cast<const double*>(c->cons_dev + off_p); }
  if (!q_on_device) { MV_HIP(hipMemcpyAsync(c->cons_dev + off_q, Q, 24 * C, hipMemcpyHostToDevice, st)); dQ = reinterpret_cast<const double*>(c->cons_dev + off_q); }
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
    hipLaunchKernelGGL(cons_hyp_kernel, grid_h, block, 0, st, dP, dQ, (int)n_pairs, (int)H, seed, s2, c->cons_count, hidx, ctl);
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
    hipLaunchKernelGGL(cons_score_kernel, dim3((unsigned int)gx, gy_u), block, 0, st, dP, dQ, (int)n_pairs, seed, s2, tau2, hidx, n_acc, per_y_i, c->cons_count);
    MV_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "cons_pick", 4.0 * NH + 49.0 * C);
    hipLaunchKernelGGL(cons_pick_kernel, grid_h, block, 0, st, c->cons_count, (int)H, ctl);
    hipLaunchKernelGGL(cons_flags_kernel, dim3((unsigned int)((C + kThreads - 1) / kThreads)), block, 0, st, dP, dQ, (int)n_pairs, seed, s2, tau2, c->cons_flags, ctl);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(&h_ctl, ctl, sizeof(ConsCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (out) *out = h_ctl.res;
  c->cons_H = H; c->cons_c = n_pairs;
  return MVICP_OK;
}

}  // namespace mvicp
