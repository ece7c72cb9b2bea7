// Consistent normal orientation without a viewpoint (mvicp_orient_normals): the signs of one cloud's normals are propagated along the
// maximum spanning forest of its neighbour graph, weighted by |N_i . N_j| (Hoppe et al. 1992), as a pure function of the stored bytes, bit
// for bit.  The contract is stated in include/mvicp.h; tests/orientref.py is its numpy form and its scalar Kruskal loop.  DESIGN.md §3.15.
// Behind it in this file: the agreement count between the normals of two clouds over the correspondence lists (mvicp_normal_agreement) and
// the negation of a frame's stored normals (mvicp_negate_normals).
//
// The graph is the rows of one internal knn_search (self mode).  The edge order (w descending, then (min index, max index) ascending) is a
// strict total order, so the forest is unique and any correct algorithm builds it; here Boruvka rounds over flat component labels:
//   orient_clear    best[r] <- (0, ~0) for every label r
//   orient_weight   every point scans its row; an edge that leaves its component proposes the bits of w to BOTH end components by a 64-bit
//                   atomic max (a row is directed: the other end may not list this point).  Non-negative doubles order as unsigned integers.
//   orient_pair     the same scan; an edge whose w is its component's maximum proposes (min index << 32 | max index) by a 64-bit atomic min
//   orient_hook     every root reads its component's best edge and hooks onto the component at the other end, with the parity
//                   x_a ^ x_b ^ [d < 0]; when both ends chose the same edge (the only cycle a strict total order allows) the lower label
//                   stays a root.  It reads the labels of this round (P) and writes the next ones (Q): no thread reads what another writes.
//   orient_jump     pointer jumping on Q, label and parity packed in ONE 32-bit word (bit 31 = parity to the parent), so that a word always
//                   holds an ancestor and the parity to it, whoever reads it when.  At most 32 jumps per launch; the launch counts the
//                   points whose parent is not yet a root, and the host repeats it while there are any.  A launch at least doubles the
//                   distance every pointer spans, so 32 launches reach any root.
// The host reads (hooks, unfinished) once per launch sequence and stops when a round made no hook.  Then
//   orient_anchor   anchor[root] <- min index (32-bit atomic min, one per wave where the wave lies in one tree)
//   orient_vote     x_i re-based on the anchor, comp[i], and the exact integer votes #(s_i < 0), #(s_i > 0) per component
//   orient_write    flip = x ^ g, the normals, the flags
// No kernel waits for another workgroup: every dependency is a kernel boundary.  Every fp64 operation is an __d*_rn intrinsic: rounded on
// its own, never contracted into an fma.
#include <climits>
#include <cstring>
#include <utility>

#include "common.h"

namespace mvicp {

namespace {

constexpr int OT = 256;
constexpr int kMaxRounds = 32, kMaxJumps = 32;
constexpr unsigned int kParity = 0x80000000u, kLabel = 0x7fffffffu;
constexpr unsigned long long kNoPair = ~0ull;
// control block (ints), all the host ever reads: [0] a non-finite weight was seen, [1] components, [2] hooks made so far, [3] the points
// that the jump launches so far left unfinished.  [2] and [3] only grow, and the host takes differences (of [3] modulo 2^32: a launch adds
// less than 2^31), so nothing is cleared between launches and one 16-byte copy answers every question.
constexpr int kCtlBad = 0, kCtlComps = 1, kCtlHooks = 2, kCtlOpen = 3, kCtlInts = 4;

typedef unsigned long long u64;

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
// d_ij: bitwise symmetric in i and j (IEEE multiplication commutes)
__device__ __forceinline__ double edge_dot(const double* __restrict__ N, int i, int j) {
  const double* a = N + 3 * (size_t)i;
  const double* b = N + 3 * (size_t)j;
  return dot3(a[0], a[1], a[2], b[0], b[1], b[2]);
}
__device__ __forceinline__ u64 pair_key(int i, int j) { return ((u64)(unsigned int)min(i, j) << 32) | (u64)(unsigned int)max(i, j); }
__device__ __forceinline__ unsigned int load_word(const unsigned int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u64 load_u64(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(OT) void orient_init_kernel(int n, unsigned int* __restrict__ P, int* __restrict__ anchor, int* __restrict__ cpos, int* __restrict__ cneg) {
  const int i = blockIdx.x * OT + threadIdx.x;
  if (i >= n) return;
  P[i] = (unsigned int)i; anchor[i] = INT_MAX; cpos[i] = 0; cneg[i] = 0;
}

__global__ __launch_bounds__(OT) void orient_clear_kernel(int n, u64* __restrict__ bestw, u64* __restrict__ bestp) {
  const int i = blockIdx.x * OT + threadIdx.x;
  if (i >= n) return;
  bestw[i] = 0; bestp[i] = kNoPair;
}

// PAIR = false: the weight pass (FIRST: every edge of the graph leaves its component, so this launch sees every weight and reports a
// non-finite one); PAIR = true: the pair pass among the edges whose weight is the maximum
template <bool PAIR, bool FIRST>
__global__ __launch_bounds__(OT) void orient_propose_kernel(int n, int k, const int* __restrict__ cnt, const int* __restrict__ idx, const double* __restrict__ N,
                                                            const unsigned int* __restrict__ P, u64* bestw, u64* bestp, int* ctl) {
  const int i = blockIdx.x * OT + threadIdx.x;
  if (i >= n) return;
  const int len = cnt[i];   // <= k
  const int ci = (int)(P[i] & kLabel);
  const double a0 = N[3 * (size_t)i], a1 = N[3 * (size_t)i + 1], a2 = N[3 * (size_t)i + 2];
  bool bad = false;
  for (int t = 0; t < len; ++t) {
    const int j = idx[(size_t)i * (size_t)k + t];   // in [0, n)
    if (j == i) continue;
    const int cj = (int)(P[j] & kLabel);
    if (ci == cj) continue;
    const double* b = N + 3 * (size_t)j;
    const double d = dot3(a0, a1, a2, b[0], b[1], b[2]);
    // a non-finite d ends the call (FIRST reports it) and proposes nothing in any pass: the bits of a NaN may differ between the two ends
    // of the edge, and only keys that both ends see alike keep the hook graph free of cycles longer than 2
    if (!(fabs(d) <= 1.79769313486231570815e308)) { bad = true; continue; }
    const u64 w = (u64)__double_as_longlong(fabs(d));
    if (!PAIR) {
      // (the plain look first: a value read there is never above the true maximum, so it can only cost an atomic that changes nothing)
      if (w > load_u64(bestw + ci)) atomicMax(bestw + ci, w);
      if (w > load_u64(bestw + cj)) atomicMax(bestw + cj, w);
    } else {
      const u64 key = pair_key(i, j);
      if (w == bestw[ci] && key < load_u64(bestp + ci)) atomicMin(bestp + ci, key);
      if (w == bestw[cj] && key < load_u64(bestp + cj)) atomicMin(bestp + cj, key);
    }
  }
  if (FIRST && bad) atomicOr(ctl + kCtlBad, 1);
}

__global__ __launch_bounds__(OT) void orient_hook_kernel(int n, const double* __restrict__ N, const unsigned int* __restrict__ P, const u64* __restrict__ bestp,
                                                         unsigned int* __restrict__ Q, int* hooks) {
  const int i = blockIdx.x * OT + threadIdx.x;
  if (i >= n) return;
  const unsigned int w = P[i];
  unsigned int out = w;
  bool hooked = false;
  if (w == (unsigned int)i) {   // a root (its parity is 0)
    const u64 key = bestp[i];
    if (key != kNoPair) {
      const int a = (int)(key >> 32), b = (int)(key & 0xffffffffu);
      const unsigned int wa = P[a], wb = P[b];
      const int ra = (int)(wa & kLabel), rb = (int)(wb & kLabel);
      const int o = ra == i ? rb : ra;   // the component at the other end
      if (!(bestp[o] == key && i < o)) {   // (both chose this edge: the lower label stays a root)
        const unsigned int f = edge_dot(N, a, b) < 0.0 ? kParity : 0u;
        out = (unsigned int)o | ((wa ^ wb ^ f) & kParity);
        hooked = true;
      }
    }
  }
  Q[i] = out;
  const u64 m = __ballot(hooked);
  if (m != 0 && (threadIdx.x & 63) == (unsigned int)__ffsll((long long)m) - 1) atomicAdd(hooks, (int)__popcll(m));
}

__global__ __launch_bounds__(OT) void orient_jump_kernel(int n, unsigned int* Q, int* unfinished) {
  const int i = blockIdx.x * OT + threadIdx.x;
  bool open = false;
  if (i < n) {
    unsigned int w = load_word(Q + i);
    for (int jump = 0; jump < kMaxJumps; ++jump) {
      const unsigned int p = w & kLabel;
      if (p == (unsigned int)i) break;                 // a root
      const unsigned int w2 = load_word(Q + p);
      if ((w2 & kLabel) == p) break;                   // the parent is a root
      w = (w2 & kLabel) | ((w ^ w2) & kParity);        // the parent's ancestor, the parities added
      __hip_atomic_store(Q + i, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned int p = w & kLabel;
    open = p != (unsigned int)i && (load_word(Q + p) & kLabel) != p;
  }
  const u64 m = __ballot(open);
  if (m != 0 && (threadIdx.x & 63) == (unsigned int)__ffsll((long long)m) - 1) atomicAdd(unfinished, (int)__popcll(m));
}

__global__ __launch_bounds__(OT) void orient_anchor_kernel(int n, const unsigned int* __restrict__ P, int* anchor) {
  const int i = blockIdx.x * OT + threadIdx.x;
  const bool in = i < n;
  const unsigned int r = in ? P[i] & kLabel : ~0u;   // (no label: a wave with lanes past the cloud takes the per-lane path)
  // a wave that lies in one tree (the common case: a cloud that is one tree queues on ONE word) sends its lowest index, which is lane 0's
  const bool uniform = __all(r == (unsigned int)__shfl((int)r, 0, 64)) != 0;
  if (in && (!uniform || (threadIdx.x & 63) == 0)) {
    int* a = anchor + r;
    if (i < __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(a, i);
  }
}

// one atomic per wave when the whole wave votes in one component (the common case), else one per voting lane
__device__ __forceinline__ void wave_count(bool on, int a, bool uniform, int* counter) {
  if (uniform) {
    const u64 m = __ballot(on);
    if (m != 0 && (threadIdx.x & 63) == (unsigned int)__ffsll((long long)m) - 1) atomicAdd(counter + a, (int)__popcll(m));
  } else if (on) {
    atomicAdd(counter + a, 1);
  }
}

__global__ __launch_bounds__(OT) void orient_vote_kernel(int n, int mode, const double* __restrict__ N, const double* __restrict__ pts, double r0, double r1, double r2,
                                                         const unsigned int* __restrict__ P, const int* __restrict__ anchor, int* __restrict__ comp,
                                                         unsigned char* __restrict__ flip, int* cpos, int* cneg, int* ctl) {
  const int i = blockIdx.x * OT + threadIdx.x;
  const bool in = i < n;
  int a = -1;
  bool neg = false, pos = false;
  if (in) {
    const unsigned int w = P[i];
    a = anchor[w & kLabel];
    const unsigned int x = (w ^ P[a]) >> 31;   // the parity to the root, re-based on the anchor
    comp[i] = a;
    flip[i] = (unsigned char)x;
    if (mode != MVICP_ORIENT_ANCHOR) {
      const double n0 = N[3 * (size_t)i], n1 = N[3 * (size_t)i + 1], n2 = N[3 * (size_t)i + 2];
      double w0 = r0, w1 = r1, w2 = r2;
      if (mode == MVICP_ORIENT_VIEWPOINT) {
        w0 = __dsub_rn(r0, pts[3 * (size_t)i]); w1 = __dsub_rn(r1, pts[3 * (size_t)i + 1]); w2 = __dsub_rn(r2, pts[3 * (size_t)i + 2]);
      }
      double s = dot3(n0, n1, n2, w0, w1, w2);
      if (x) s = -s;
      neg = s < 0.0; pos = s > 0.0;
    }
  }
  const int a0 = __shfl(a, 0, 64);
  const bool uniform = __all(a == a0) != 0;   // (lanes past the cloud carry -1: a wave with any of them takes the per-lane path, where they vote for nothing)
  wave_count(neg, a, uniform, cneg);
  wave_count(pos, a, uniform, cpos);
  const u64 m = __ballot(in && a == i);
  if (m != 0 && (threadIdx.x & 63) == (unsigned int)__ffsll((long long)m) - 1) atomicAdd(ctl + kCtlComps, (int)__popcll(m));
}

__global__ __launch_bounds__(OT) void orient_write_kernel(int n, const double* __restrict__ N, const int* __restrict__ comp, const int* __restrict__ cpos,
                                                          const int* __restrict__ cneg, unsigned char* __restrict__ flip, double* __restrict__ nrm) {
  const int i = blockIdx.x * OT + threadIdx.x;
  if (i >= n) return;
  const int a = comp[i];
  const unsigned int g = cneg[a] > cpos[a] ? 1u : 0u;   // (a tie keeps the sign)
  const unsigned int fl = (unsigned int)flip[i] ^ g;
  flip[i] = (unsigned char)fl;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const double v = N[3 * (size_t)i + t];
    nrm[3 * (size_t)i + t] = fl ? -v : v;
  }
}

__global__ __launch_bounds__(OT) void negate_kernel(size_t m, double* __restrict__ nor, double* __restrict__ snor) {
  const size_t i = (size_t)blockIdx.x * OT + threadIdx.x;
  if (i >= m) return;
  nor[i] = -nor[i];
  snor[i] = -snor[i];
}

// a = R_src N_first, b = R_dst N_second with the rotation rows of the two poses (16 column-major doubles), t = a . b
constexpr int kAgreeBlocks = 64;   // workgroups per edge (grid-stride over the list)
__global__ __launch_bounds__(OT) void agreement_kernel(const int* __restrict__ cnt, const long long* __restrict__ cap_off, const int* __restrict__ first,
                                                       const int* __restrict__ second, const double* const* __restrict__ nor_src,
                                                       const double* const* __restrict__ nor_dst, const int* __restrict__ esrc, const int* __restrict__ edst,
                                                       const double* __restrict__ poses, int* pos, int* neg) {
  const int e = blockIdx.x / kAgreeBlocks, part = blockIdx.x % kAgreeBlocks;
  const int m = cnt[e];
  if (part * OT >= m) return;   // (block-uniform)
  const double* Ps = poses + 16 * (size_t)esrc[e];
  const double* Pd = poses + 16 * (size_t)edst[e];
  const double* ns = nor_src[e];
  const double* nd = nor_dst[e];
  const size_t base = (size_t)cap_off[e];
  int np = 0, nn = 0;
  for (int t = part * OT + threadIdx.x; t < m; t += kAgreeBlocks * OT) {
    const double* x = ns + 3 * (size_t)first[base + t];    // sorted positions, < N_src
    const double* y = nd + 3 * (size_t)second[base + t];   // sorted positions, < N_dst
    const double a0 = dot3(Ps[0], Ps[4], Ps[8], x[0], x[1], x[2]), a1 = dot3(Ps[1], Ps[5], Ps[9], x[0], x[1], x[2]), a2 = dot3(Ps[2], Ps[6], Ps[10], x[0], x[1], x[2]);
    const double b0 = dot3(Pd[0], Pd[4], Pd[8], y[0], y[1], y[2]), b1 = dot3(Pd[1], Pd[5], Pd[9], y[0], y[1], y[2]), b2 = dot3(Pd[2], Pd[6], Pd[10], y[0], y[1], y[2]);
    const double d = dot3(a0, a1, a2, b0, b1, b2);
    np += d > 0.0; nn += d < 0.0;
  }
  // integer sums: any order gives the same count
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) { np += __shfl_xor(np, s, 64); nn += __shfl_xor(nn, s, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (np) atomicAdd(pos + e, np);
    if (nn) atomicAdd(neg + e, nn);
  }
}

}  // namespace

long long orient_normals(mvicp_ctx* c, const FrameDev& f, const double* N, int k, double radius, double B2, int mode, const double* ref) {
  c->ori.drop_result();   // (the last result ends here; a failed call leaves none behind)
  const long long total = knn_search(c, f, nullptr, 0, 0, k, radius, B2);
  if (total < 0) return total;
  const int n = f.n;
  if (n == 0) { c->ori.rows = 0; return 0; }
  hipStream_t st = c->stream;
  const size_t Nn = (size_t)n;
  // [nrm | comp | flip | P | Q | bestw | bestp | anchor | cpos | cneg | ctl]
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off += align256(bytes); return at; };
  const size_t o_nrm = take(24 * Nn), o_comp = take(4 * Nn), o_flip = take(Nn), o_P = take(4 * Nn), o_Q = take(4 * Nn), o_bw = take(8 * Nn), o_bp = take(8 * Nn),
               o_anchor = take(4 * Nn), o_cpos = take(4 * Nn), o_cneg = take(4 * Nn), o_ctl = take(sizeof(int) * kCtlInts);
  MV_CHECK(c->ori.dev.reserve(off));
  MV_CHECK(c->ori.pin.reserve(sizeof(int) * kCtlInts));
  char* base = c->ori.dev.p;
  c->ori.nrm = reinterpret_cast<double*>(base + o_nrm);
  c->ori.comp = reinterpret_cast<int*>(base + o_comp);
  c->ori.flip = reinterpret_cast<unsigned char*>(base + o_flip);
  unsigned int* P = reinterpret_cast<unsigned int*>(base + o_P);
  unsigned int* Q = reinterpret_cast<unsigned int*>(base + o_Q);
  u64* bestw = reinterpret_cast<u64*>(base + o_bw);
  u64* bestp = reinterpret_cast<u64*>(base + o_bp);
  int* anchor = reinterpret_cast<int*>(base + o_anchor);
  int* cpos = reinterpret_cast<int*>(base + o_cpos);
  int* cneg = reinterpret_cast<int*>(base + o_cneg);
  int* ctl = reinterpret_cast<int*>(base + o_ctl);
  int* h_ctl = reinterpret_cast<int*>(c->ori.pin.p);
  const dim3 grid((unsigned int)grid_of(n, OT)), block(OT);
  const int* cnt = c->knn.cnt;
  const int* idx = c->knn.idx;
  MV_HIP(hipMemsetAsync(ctl, 0, sizeof(int) * kCtlInts, st));
  hipLaunchKernelGGL(orient_init_kernel, grid, block, 0, st, n, P, anchor, cpos, cneg);
  MV_HIP(hipGetLastError());
  int hooks_seen = 0;
  unsigned int open_seen = 0;
  bool done = false;
  for (int round = 0; round < kMaxRounds && !done; ++round) {
    {
      // per point and pass its row of indices, its label and normal, per entry a label and a normal; the atomics are not counted
      ProfScope ps(c, "orient_round", 2.0 * ((4.0 + 4.0 + 24.0 + 4.0 * k) * n + 28.0 * (double)total) + 40.0 * n);
      hipLaunchKernelGGL(orient_clear_kernel, grid, block, 0, st, n, bestw, bestp);
      if (round == 0) hipLaunchKernelGGL((orient_propose_kernel<false, true>), grid, block, 0, st, n, k, cnt, idx, N, P, bestw, bestp, ctl);
      else hipLaunchKernelGGL((orient_propose_kernel<false, false>), grid, block, 0, st, n, k, cnt, idx, N, P, bestw, bestp, ctl);
      hipLaunchKernelGGL((orient_propose_kernel<true, false>), grid, block, 0, st, n, k, cnt, idx, N, P, bestw, bestp, ctl);
      hipLaunchKernelGGL(orient_hook_kernel, grid, block, 0, st, n, N, P, bestp, Q, ctl + kCtlHooks);
      MV_HIP(hipGetLastError());
    }
    // pointer jumping until every point's parent is a root
    for (int jumps = 0;; ++jumps) {
      if (jumps >= kMaxJumps) { set_error("orient_normals: the labels did not settle in %d jump launches", kMaxJumps); return MVICP_ERR_INTERNAL; }
      {
        ProfScope ps(c, "orient_round", 12.0 * n);
        hipLaunchKernelGGL(orient_jump_kernel, grid, block, 0, st, n, Q, ctl + kCtlOpen);
        MV_HIP(hipGetLastError());
      }
      MV_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(int) * kCtlInts, hipMemcpyDeviceToHost, st));
      MV_HIP(hipStreamSynchronize(st));
      // (the normals are judged before the labels: what a non-finite weight does to the labels is the caller's error, not an internal one)
      if (h_ctl[kCtlBad]) { set_error("a non-finite dot of two normals: the normals of the frame are not finite"); return MVICP_ERR_ARG; }
      const unsigned int open = (unsigned int)h_ctl[kCtlOpen] - open_seen;
      open_seen = (unsigned int)h_ctl[kCtlOpen];
      if (open == 0) break;
    }
    if (h_ctl[kCtlHooks] == hooks_seen) done = true;
    hooks_seen = h_ctl[kCtlHooks];
    std::swap(P, Q);
  }
  if (!done) { set_error("orient_normals: the forest did not close in %d rounds", kMaxRounds); return MVICP_ERR_INTERNAL; }
  {
    ProfScope ps(c, "orient_finish", (4.0 + 8.0 + 24.0 + 24.0 + 5.0 + 5.0 + 24.0 + 24.0) * n);
    hipLaunchKernelGGL(orient_anchor_kernel, grid, block, 0, st, n, P, anchor);
    hipLaunchKernelGGL(orient_vote_kernel, grid, block, 0, st, n, mode, N, f.pts, ref[0], ref[1], ref[2], P, anchor, c->ori.comp, c->ori.flip, cpos, cneg, ctl);
    hipLaunchKernelGGL(orient_write_kernel, grid, block, 0, st, n, N, c->ori.comp, cpos, cneg, c->ori.flip, c->ori.nrm);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(int) * kCtlInts, hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  c->ori.rows = n;
  c->ori.comps = h_ctl[kCtlComps];
  return c->ori.comps;
}

int negate_normals(mvicp_ctx* c, FrameDev& f) {
  const size_t m = 3 * (size_t)f.n;
  if (m) {
    hipLaunchKernelGGL(negate_kernel, dim3((unsigned int)((m + OT - 1) / OT)), dim3(OT), 0, c->stream, m, f.nor, f.grid.snor);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
}

int normal_agreement(mvicp_ctx* c, const double* poses, const char* use, int* pos, int* neg) {
  const int E = c->E, K = c->n_frames;
  const size_t Es = (size_t)E;
  // host image of [poses K x 16 doubles | nor_src E pointers | nor_dst E pointers | cnt E ints], behind it on the device [pos E ints | neg E ints]
  const size_t o_ps = 0, o_ns = o_ps + align256(128 * (size_t)K), o_nd = o_ns + align256(sizeof(void*) * Es), o_cnt = o_nd + align256(sizeof(void*) * Es),
               o_out = o_cnt + align256(4 * Es), bytes = o_out + 8 * Es;
  MV_CHECK(c->agree.dev.reserve(bytes));
  MV_CHECK(c->agree.pin.reserve(bytes));
  char* h = c->agree.pin.p;
  char* d = c->agree.dev.p;
  std::memcpy(h + o_ps, poses, 128 * (size_t)K);
  const double** ns = reinterpret_cast<const double**>(h + o_ns);
  const double** nd = reinterpret_cast<const double**>(h + o_nd);
  int* cnt = reinterpret_cast<int*>(h + o_cnt);
  bool any = false;
  for (int e = 0; e < E; ++e) {
    cnt[e] = use[e] ? c->hist.h_count[e] : 0;
    ns[e] = c->frames[c->esrc[e]].grid.snor; nd[e] = c->frames[c->edst[e]].grid.snor;
    any = any || cnt[e] > 0;
  }
  hipStream_t st = c->stream;
  MV_HIP(hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, st));
  MV_HIP(hipMemsetAsync(d + o_out, 0, 8 * Es, st));
  if (any) {
    ProfScope ps(c, "normal_agreement", 0.0);
    hipLaunchKernelGGL(agreement_kernel, dim3((unsigned int)(Es * kAgreeBlocks)), dim3(OT), 0, st, reinterpret_cast<const int*>(d + o_cnt), c->d_cap_off,
                       (const int*)c->d_first, (const int*)c->d_second, reinterpret_cast<const double* const*>(d + o_ns),
                       reinterpret_cast<const double* const*>(d + o_nd), (const int*)c->d_esrc, (const int*)c->d_edst, reinterpret_cast<const double*>(d + o_ps),
                       reinterpret_cast<int*>(d + o_out), reinterpret_cast<int*>(d + o_out) + E);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(h + o_out, d + o_out, 8 * Es, hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  const int* out = reinterpret_cast<const int*>(h + o_out);
  for (int e = 0; e < E; ++e) { if (pos) pos[e] = out[e]; if (neg) neg[e] = out[E + e]; }
  return MVICP_OK;
}

}  // namespace mvicp
