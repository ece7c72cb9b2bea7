// K3/K4 — cutoff filter + stable compaction, packed-stream gather, exact median (anchored two-pass select / bracket select).
//
// Replaces the tail of Frame::computeClosestPointsToNeighbours (src/internal/frame.cpp:156-176):
//   if (sqrt(d2) < thresh) push {k, idx, dist}        -> flag / exclusive scan / scatter, ascending k
//   nth_element(dists, size/2); weight = 1.5 * median -> select on the fp64 bit pattern of d2
// The acceptance test is evaluated as `d2 < bound` where the host has computed `bound` = the smallest
// double whose correctly rounded sqrt is >= (double)thresh, so the decision is bit-identical to the
// reference's `sqrt(d2) < thresh` without a device sqrt.  sqrt is monotone, so the median of the
// distances is the sqrt of the median of d2; the host takes that one sqrt (IEEE, exact).
// With reject masks (mvicp_set_reject_mask) the test is list_accepts (nn_list.h): the cutoff AND neither end flagged; everything below --
// scan, scatter, gather, select, scale -- then runs over the kept pairs alone.
//
// The gather kernel also materialises, once per ICP round, the per-correspondence operand stream the
// LM evaluations re-read up to ~100 times: SoA p (3) | n (3) | c = n . q | q (3), 10 arrays, of which point-to-plane
// streams 7 (56 B per correspondence) and point-to-point 6 — instead of 2-3 random 24-B gathers per evaluation.
#include "common.h"
#include "nn_list.h"

#include <cstring>

namespace mvicp {

namespace {

constexpr int NT = 256;
constexpr int IPT = kCompactBlock / NT;  // 4 consecutive queries per thread

__device__ __forceinline__ int find_edge(const int* __restrict__ off, int E, int b) {
  int lo = 0, hi = E;  // largest e with off[e] <= b
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int block_exclusive_scan(int v, int* __restrict__ wave_tot, int* total) {
  // inclusive scan inside the wave (64 lanes) by shuffles, then across the 4 waves through LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int t = wave_tot[w];
    if (w < wave) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - v;
}

// The reject masks of edge e (mvicp_set_reject_mask): mask_tab = E source-side pointers, then E target-side ones, each the frame's mask in
// sorted order or null; mask_tab itself is null while no frame has a mask, so a maskless search pays one wave-uniform branch per workgroup.
struct EdgeMasks { const unsigned char* src; const unsigned char* dst; };
__device__ __forceinline__ EdgeMasks edge_masks(const unsigned char* const* __restrict__ mask_tab, int E, int e) {
  EdgeMasks m = {nullptr, nullptr};
  if (mask_tab != nullptr) { m.src = mask_tab[e]; m.dst = mask_tab[E + e]; }
  return m;
}

__global__ __launch_bounds__(NT) void count_kernel(const int* __restrict__ cblock_off, int E, const int* __restrict__ nsrc,
                                                   const long long* __restrict__ cap_off, const int* __restrict__ nn_idx,
                                                   const double* __restrict__ nn_d2, double bound, int* __restrict__ cblock_cnt,
                                                   const int* __restrict__ dirty, const unsigned char* const* __restrict__ mask_tab) {
  __shared__ int wave_tot[NT / 64];
  const int b = blockIdx.x;
  const int e = find_edge(cblock_off, E, b);
  if (dirty[e] == 0) return;  // list unchanged since last round
  const int lb = b - cblock_off[e];
  const int n = nsrc[e];
  const long long base = cap_off[e];
  const EdgeMasks m = edge_masks(mask_tab, E, e);
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int k = lb * kCompactBlock + threadIdx.x * IPT + i;
    if (k < n) cnt += list_accepts(k, nn_idx[base + k], nn_d2[base + k], bound, m.src, m.dst) ? 1 : 0;
  }
  int total;
  block_exclusive_scan(cnt, wave_tot, &total);
  if (threadIdx.x == 0) cblock_cnt[b] = total;
}

// one workgroup per edge: exclusive scan of its block counts (<= ~1k blocks for 1M points), in place.
__global__ __launch_bounds__(NT) void scan_kernel(const int* __restrict__ cblock_off, int* __restrict__ cblock_cnt, int* __restrict__ count,
                                                  const int* __restrict__ dirty) {
  __shared__ int wave_tot[NT / 64];
  __shared__ int carry_s;
  const int e = blockIdx.x;
  if (dirty[e] == 0) return;
  const int b0 = cblock_off[e], b1 = cblock_off[e + 1];
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int s = b0; s < b1; s += NT) {
    const int b = s + threadIdx.x;
    const int v = (b < b1) ? cblock_cnt[b] : 0;
    int total;
    const int ex = block_exclusive_scan(v, wave_tot, &total);
    const int carry = carry_s;
    if (b < b1) cblock_cnt[b] = carry + ex;
    __syncthreads();
    if (threadIdx.x == 0) carry_s = carry + total;
    __syncthreads();
  }
  if (threadIdx.x == 0) count[e] = carry_s;
}

__global__ __launch_bounds__(NT) void scatter_kernel(const int* __restrict__ cblock_off, int E, const int* __restrict__ nsrc,
                                                     const long long* __restrict__ cap_off, const int* __restrict__ nn_idx,
                                                     const double* __restrict__ nn_d2, double bound, const int* __restrict__ cblock_cnt,
                                                     int* __restrict__ first, int* __restrict__ second, double* __restrict__ cd2,
                                                     int* __restrict__ qpos, const int* __restrict__ dirty,
                                                     const unsigned char* const* __restrict__ mask_tab) {
  __shared__ int wave_tot[NT / 64];
  const int b = blockIdx.x;
  const int e = find_edge(cblock_off, E, b);
  if (dirty[e] == 0) return;
  const int lb = b - cblock_off[e];
  const int n = nsrc[e];
  const long long base = cap_off[e];
  const EdgeMasks m = edge_masks(mask_tab, E, e);
  int idx[IPT];
  double d2[IPT];
  bool ok[IPT];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int k = lb * kCompactBlock + threadIdx.x * IPT + i;
    ok[i] = false;
    if (k < n) {
      idx[i] = nn_idx[base + k];
      d2[i] = nn_d2[base + k];
      ok[i] = list_accepts(k, idx[i], d2[i], bound, m.src, m.dst);
    }
    cnt += ok[i] ? 1 : 0;
  }
  int total;
  int pos = cblock_cnt[b] + block_exclusive_scan(cnt, wave_tot, &total);
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int k = lb * kCompactBlock + threadIdx.x * IPT + i;
    if (k < n) qpos[base + k] = ok[i] ? pos : -1;
    if (!ok[i]) continue;
    first[base + pos] = k;
    second[base + pos] = idx[i];
    cd2[base + pos] = d2[i];
    ++pos;
  }
}

// A frame's reject mask from original into sorted order, so that the acceptance test reads one byte at the index it already holds:
// smask[i] = omask[sidx[i]], four sorted positions per thread (one 16-B index load, four byte gathers, one 4-B store; smask comes from
// hipMalloc, so its words are aligned).  Every access is bounded by n.
__global__ __launch_bounds__(NT) void mask_permute_kernel(const unsigned char* __restrict__ omask, const int* __restrict__ sidx, int n,
                                                          unsigned char* __restrict__ smask) {
  const long long i = 4ll * ((long long)blockIdx.x * NT + threadIdx.x);
  if (i + 3 < n) {
    const int4 s = *reinterpret_cast<const int4*>(sidx + i);
    const unsigned int w = (unsigned int)omask[s.x] | ((unsigned int)omask[s.y] << 8) | ((unsigned int)omask[s.z] << 16) | ((unsigned int)omask[s.w] << 24);
    *reinterpret_cast<unsigned int*>(smask + i) = w;
  } else {
    for (long long k = i; k < n; ++k) smask[k] = omask[sidx[k]];
  }
}

// packed operand stream for the LM evaluations
__global__ __launch_bounds__(NT) void gather_kernel(const int* __restrict__ cblock_off, int E, const int* __restrict__ count,
                                                    const long long* __restrict__ cap_off, long long total_cap, const int* __restrict__ first,
                                                    const int* __restrict__ second, const PointRec* const* __restrict__ src_rec,
                                                    const PointRec* const* __restrict__ dst_rec, const double* const* __restrict__ dst_nor,
                                                    double* __restrict__ stream, const int* __restrict__ dirty) {
  const int b = blockIdx.x;
  const int e = find_edge(cblock_off, E, b);
  if (dirty[e] == 0) return;  // same list -> same operands
  const int lb = b - cblock_off[e];
  const int cnt = count[e];
  if (lb * kCompactBlock >= cnt) return;
  const long long base = cap_off[e];
  const PointRec* __restrict__ sp = src_rec[e];   // first / second are SORTED positions: neighbouring correspondences
  const PointRec* __restrict__ dp = dst_rec[e];   // read neighbouring records (coherent gathers)
  const double* __restrict__ dn = dst_nor[e];
  for (int i = 0; i < IPT; ++i) {
    const int pos = lb * kCompactBlock + i * NT + threadIdx.x;
    if (pos >= cnt) break;
    const size_t f = (size_t)first[base + pos], s = (size_t)second[base + pos];
    const size_t o = (size_t)(base + pos);
    const double2* pa = reinterpret_cast<const double2*>(sp + f);
    const double2 a0 = pa[0], a1 = pa[1];
    const double2* pb = reinterpret_cast<const double2*>(dp + s);
    const double2 b0 = pb[0], b1 = pb[1];
    // arrays: 0-2 p | 3-5 n | 6 c = n . q | 7-9 q   (linearize.hip: point-to-plane reads 0..6, point-to-point 0-2 and 7-9)
    __builtin_nontemporal_store(a0.x, &stream[0 * total_cap + o]);
    __builtin_nontemporal_store(a0.y, &stream[1 * total_cap + o]);
    __builtin_nontemporal_store(a1.x, &stream[2 * total_cap + o]);
    __builtin_nontemporal_store(b0.x, &stream[7 * total_cap + o]);
    __builtin_nontemporal_store(b0.y, &stream[8 * total_cap + o]);
    __builtin_nontemporal_store(b1.x, &stream[9 * total_cap + o]);
    if (dn != nullptr) {
      const double n0 = dn[3 * s], n1 = dn[3 * s + 1], n2 = dn[3 * s + 2];
      __builtin_nontemporal_store(n0, &stream[3 * total_cap + o]);
      __builtin_nontemporal_store(n1, &stream[4 * total_cap + o]);
      __builtin_nontemporal_store(n2, &stream[5 * total_cap + o]);
      __builtin_nontemporal_store(n0 * b0.x + n1 * b0.y + n2 * b1.x, &stream[6 * total_cap + o]);
    }
  }
}

// ---- exact median of the accepted d2 of an edge: select on the fp64 bit pattern, two streaming passes ---------------------
// d2 >= 0, so bit 63 is clear and the unsigned pattern is monotone in the value.  Every accepted key lies below the acceptance
// bound, so the first digit is anchored there instead of spending 11 bits on an exponent field that hardly varies:
//   bin(key) = clamp(2047 - ((kb >> SH) - (key >> SH)), 0, 2047),   kb = pattern of the bound, SH = 46: a bin is 1/64 octave of d2,
// 2048 bins reach 32 octaves below the bound; whatever lies further down shares bin 0, whatever lies at or above the bound bin 2047.
// The function is monotone non-decreasing in the key — all exactness needs.  select_hist_kernel histograms every key (one read),
// select_pick_kernel (one workgroup per edge; a "last workgroup picks" ticket scheme needs an agent-scope fence per workgroup, which
// on the 8-XCD part writes back / invalidates L2 and made the select 4x slower) finds the bin that holds rank size/2 and writes the
// bin's smallest and largest pattern as the edge's bracket; bracket_pass_kernel / bracket_final_kernel (below) then count the keys
// under the bracket, compact the bin (a second read) and select inside it — by construction the rank is inside.  Exact for any
// input: all-equal keys or a cutoff far above every key only make the compacted bin as long as the list.
constexpr int kSelBins = 2048;
constexpr int kSelShift = 46;

__device__ __forceinline__ unsigned int sel_bin(unsigned long long key, long long kbq) {
  const long long d = kbq - (long long)(key >> kSelShift);
  return d <= 0 ? (unsigned int)(kSelBins - 1) : d >= kSelBins - 1 ? 0u : (unsigned int)(kSelBins - 1 - d);
}

// Workgroup-wide: which of `nbins` bins (nbins = NT * PER) holds rank k, and how many keys sit in the bins below it.
// `get(bin)` returns the count of a bin.  All NT threads must call; result valid in every thread.
template <int PER, typename F>
__device__ __forceinline__ void pick_bin(F get, unsigned int k, int* __restrict__ wave_tot, int* __restrict__ sh_pick, int& bin, unsigned int& below) {
  unsigned int h[PER];
  int mine = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { h[i] = get(threadIdx.x * PER + i); mine += (int)h[i]; }
  int total;
  const int ex = block_exclusive_scan(mine, wave_tot, &total);
  if (threadIdx.x == 0) { sh_pick[0] = NT * PER - 1; sh_pick[1] = total; }   // unreachable default (k < total always)
  __syncthreads();
  if ((unsigned int)ex <= k && k < (unsigned int)(ex + mine)) {
    unsigned int cum = (unsigned int)ex;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (cum + h[i] > k) { sh_pick[0] = threadIdx.x * PER + i; sh_pick[1] = (int)cum; break; }
      cum += h[i];
    }
  }
  __syncthreads();
  bin = sh_pick[0]; below = (unsigned int)sh_pick[1];
  __syncthreads();
}

// histogram of the anchored first digit: one streaming read of the keys (16 B per lane per load), counted in LDS, one global atomic
// per non-empty bin and workgroup.  (The keys of a wave spread over many bins — hundreds are populated on a registration's d2 — so
// the interleaved LDS copies the exponent digit needed are gone.)
__global__ __launch_bounds__(NT) void select_hist_kernel(const int* __restrict__ sblock_off, int E, const int* __restrict__ count,
                                                         const long long* __restrict__ cap_off, const double* __restrict__ keys,
                                                         long long kbq, unsigned int* __restrict__ hist) {
  constexpr int SPT = kSelBlock / NT;   // keys per thread, two per step
  __shared__ unsigned int lh[kSelBins];
  const int b = blockIdx.x;
  const int e = find_edge(sblock_off, E, b);
  const int lb = b - sblock_off[e];
  const int cnt = count[e];
  if ((long long)lb * kSelBlock >= cnt) return;
  for (int i = threadIdx.x; i < kSelBins; i += NT) lh[i] = 0u;
  __syncthreads();
  const long long base = cap_off[e];   // multiple of 64 keys: 16-B aligned pairs
#pragma unroll
  for (int i = 0; i < SPT / 2; ++i) {
    const int pos = lb * kSelBlock + 2 * (i * NT + threadIdx.x);
    if (pos + 1 < cnt) {
      typedef double d2v __attribute__((ext_vector_type(2)));
      const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(keys + base + pos));
      atomicAdd(&lh[sel_bin((unsigned long long)__double_as_longlong(v.x), kbq)], 1u);
      atomicAdd(&lh[sel_bin((unsigned long long)__double_as_longlong(v.y), kbq)], 1u);
    } else if (pos < cnt) {
      atomicAdd(&lh[sel_bin((unsigned long long)__double_as_longlong(keys[base + pos]), kbq)], 1u);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSelBins; i += NT) {
    const unsigned int v = lh[i];
    if (v) atomicAdd(&hist[(size_t)e * kSelBins + i], v);
  }
}

// one workgroup per edge over the finished histogram: the bin of rank size/2 (dists.begin() + size()/2, frame.cpp:166) becomes the
// edge's bracket [smallest, largest pattern of the bin]; the row is left zeroed for the next search.
__global__ __launch_bounds__(NT) void select_pick_kernel(int E, const int* __restrict__ count, unsigned int* __restrict__ hist, long long kbq,
                                                         double* __restrict__ lohi) {
  __shared__ int wave_tot[NT / 64];
  __shared__ int sh_pick[2];
  const int e = blockIdx.x;
  const int cnt = count[e];
  if (cnt <= 0) {   // (no workgroup of the histogram pass touched the row)
    if (threadIdx.x == 0) { lohi[2 * e] = 0.0; lohi[2 * e + 1] = 0.0; }
    return;
  }
  unsigned int* hp = hist + (size_t)e * kSelBins;
  int bin; unsigned int below;
  pick_bin<kSelBins / NT>([&](int i) { return hp[i]; }, (unsigned int)(cnt / 2), wave_tot, sh_pick, bin, below);
#pragma unroll
  for (int i = 0; i < kSelBins / NT; ++i) hp[threadIdx.x * (kSelBins / NT) + i] = 0u;
  if (threadIdx.x == 0) {
    const long long q = kbq - (long long)(kSelBins - 1 - bin);   // key >> SH of the bin's keys (bins 1..2046); a non-empty bin has q >= 0
    const unsigned long long low_mask = (1ull << kSelShift) - 1ull;
    unsigned long long lo = 0ull, hi = 0ull;
    if (bin == kSelBins - 1) { lo = (unsigned long long)(kbq > 0 ? kbq : 0) << kSelShift; hi = 0x7FFFFFFFFFFFFFFFull; }
    else if (bin == 0) { lo = 0ull; hi = q >= 0 ? (((unsigned long long)q << kSelShift) | low_mask) : 0ull; }
    else if (q >= 0) { lo = (unsigned long long)q << kSelShift; hi = lo | low_mask; }
    lohi[2 * e] = __longlong_as_double((long long)lo); lohi[2 * e + 1] = __longlong_as_double((long long)hi);
  }
}

// SoftLOne scale of an edge on the device: a = (double)(float)(1.5 * sqrt(median d2)) — OutgoingEdge::weight (frame.cpp:168-176) widened
// the way Ceres reads it (icp-ceres.cpp:284,374,449).  Lets the first LM evaluation of the round be queued before the host has
// seen the median; the host recomputes the weight with its own IEEE sqrt and only trusts that evaluation if the two agree bit for bit.
__device__ __forceinline__ void write_a_scale(int cnt, double med, int e, double* __restrict__ a_dev, double* __restrict__ a_host) {
  if (a_dev == nullptr) return;
  const double a = cnt > 0 ? (double)(float)__dmul_rn(sqrt(med), 1.5) : 0.0;
  a_dev[e] = a;
  if (a_host) a_host[e] = a;
}

// ---- bracket select: when the registration has settled, the median of an edge barely moves between rounds.  ONE pass
// over the keys counts those below a bracket [lo, hi] around last round's median and compacts the few per cent inside it;
// one workgroup per edge then selects the wanted rank among the compacted keys in LDS.  Exact whenever the rank falls inside
// the bracket; otherwise the edge's result slot is flagged (median = -1) and the host runs the full select (launch_select_median),
// which puts the very same two kernels behind a device-made bracket that cannot miss.  Also hands (count, median d2) to the host
// through the mapped result buffer.
__global__ __launch_bounds__(NT) void bracket_pass_kernel(const int* __restrict__ sblock_off, int E, const int* __restrict__ count,
                                                          const long long* __restrict__ cap_off, const double* __restrict__ keys,
                                                          const double* __restrict__ lohi, unsigned int* __restrict__ cnt_lt,
                                                          double* __restrict__ out_keys, unsigned int* __restrict__ out_cnt) {
  // One streaming read of the keys, 16 B per lane per load; no workgroup scans: the count below the bracket is a popcount per wave,
  // the rare keys inside the bracket (about 1 %) get their slot from an LDS counter, and each workgroup touches the two per-edge
  // global counters once (hot-address atomics per wave were measured 4x slower than the whole pass).
  constexpr int SPT = kSelBlock / NT;   // keys per thread, two per step
  __shared__ unsigned int s_lt[NT / 64];
  __shared__ unsigned int s_mid, s_base;
  const int b = blockIdx.x;
  const int e = find_edge(sblock_off, E, b);
  const int lb = b - sblock_off[e];
  const int cnt = count[e];
  if ((long long)lb * kSelBlock >= cnt) return;
  if (threadIdx.x == 0) s_mid = 0u;
  __syncthreads();
  const unsigned long long lo = (unsigned long long)__double_as_longlong(lohi[2 * e]), hi = (unsigned long long)__double_as_longlong(lohi[2 * e + 1]);
  const long long base = cap_off[e];   // multiple of 64 keys: 16-B aligned pairs
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int nlt = 0, nmid = 0;
  unsigned long long kept[SPT];
#pragma unroll
  for (int i = 0; i < SPT / 2; ++i) {
    const int pos = lb * kSelBlock + 2 * (i * NT + threadIdx.x);
    unsigned long long k0 = ~0ull, k1 = ~0ull;   // ~0: not a key (d2 >= 0 has bit 63 clear)
    if (pos + 1 < cnt) {
      typedef double d2v __attribute__((ext_vector_type(2)));
      const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(keys + base + pos));
      k0 = (unsigned long long)__double_as_longlong(v.x); k1 = (unsigned long long)__double_as_longlong(v.y);
    } else if (pos < cnt) {
      k0 = (unsigned long long)__double_as_longlong(keys[base + pos]);
    }
    nlt += (k0 < lo ? 1u : 0u) + (k1 < lo ? 1u : 0u);
    const bool m0 = k0 >= lo && k0 <= hi, m1 = k1 >= lo && k1 <= hi;   // (~0 > hi always)
    kept[2 * i] = m0 ? k0 : ~0ull; kept[2 * i + 1] = m1 ? k1 : ~0ull;
    nmid += (m0 ? 1u : 0u) + (m1 ? 1u : 0u);
  }
  unsigned int off = nmid ? atomicAdd(&s_mid, nmid) : 0u;   // LDS
  unsigned int w = nlt;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);
  if (lane == 0) s_lt[wave] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int t = s_lt[0] + s_lt[1] + s_lt[2] + s_lt[3];
    if (t) atomicAdd(&cnt_lt[e], t);
    s_base = s_mid ? atomicAdd(&out_cnt[e], s_mid) : 0u;
  }
  __syncthreads();
  if (nmid) {
    off += s_base;
#pragma unroll
    for (int i = 0; i < SPT; ++i)
      if (kept[i] != ~0ull) out_keys[base + off++] = __longlong_as_double((long long)kept[i]);
  }
}

__global__ __launch_bounds__(NT) void bracket_final_kernel(int E, const int* __restrict__ count, const long long* __restrict__ cap_off,
                                                           const double* __restrict__ keys1, unsigned int* __restrict__ cnt_lt,
                                                           unsigned int* __restrict__ cnt_mid, double* __restrict__ median,
                                                           double* __restrict__ host_res, double* __restrict__ a_dev, double* __restrict__ a_host, double armed) {
  __shared__ unsigned int lh[kSelBins];
  __shared__ int wave_tot[NT / 64];
  __shared__ int sh_pick[2];
  const int e = blockIdx.x;
  const int cnt = count[e];
  double med = 0.0;
  bool ok = true;
  if (cnt > 0) {
    const unsigned int k = (unsigned int)(cnt / 2), nlt = cnt_lt[e], nmid = cnt_mid[e];
    ok = nlt <= k && k < nlt + nmid;
    if (ok) {
      unsigned long long prefix = 0ull;
      unsigned int rank = k - nlt;
      const long long base = cap_off[e];
      // the compacted keys are few (about 1 % of the list): keep them in registers across the 6 digit passes
      constexpr int KR = 8;
      const bool in_regs = nmid <= (unsigned int)(KR * NT);
      unsigned long long kreg[KR];
#pragma unroll
      for (int i = 0; i < KR; ++i) {
        const unsigned int pos = threadIdx.x + i * NT;
        kreg[i] = (in_regs && pos < nmid) ? (unsigned long long)__double_as_longlong(keys1[base + pos]) : ~0ull;
      }
      // 63 key bits, MSB first: 11 + 11 + 11 + 10 + 10 + 10
      int hi_bit = 63;
#pragma unroll 1
      for (int pass = 0; pass < 6; ++pass) {
        const int bits = pass < 3 ? 11 : 10;
        const int shift = hi_bit - bits;
        for (int i = threadIdx.x; i < kSelBins; i += NT) lh[i] = 0u;
        __syncthreads();
        if (in_regs) {
#pragma unroll
          for (int i = 0; i < KR; ++i) {   // (~0 never matches: bit 63 of the prefix is clear)
            const unsigned long long key = kreg[i];
            if ((key >> hi_bit) == (prefix >> hi_bit)) atomicAdd(&lh[(key >> shift) & ((1ull << bits) - 1ull)], 1u);
          }
        } else {
          for (unsigned int pos = threadIdx.x; pos < nmid; pos += NT) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(keys1[base + pos]);
            if ((key >> hi_bit) == (prefix >> hi_bit)) atomicAdd(&lh[(key >> shift) & ((1ull << bits) - 1ull)], 1u);
          }
        }
        __syncthreads();
        int bin; unsigned int below;
        pick_bin<kSelBins / NT>([&](int i) { return lh[i]; }, rank, wave_tot, sh_pick, bin, below);
        prefix |= (unsigned long long)bin << shift;
        rank -= below;
        hi_bit = shift;
      }
      med = __longlong_as_double((long long)prefix);
    }
  }
  if (threadIdx.x == 0) {
    if (ok) median[e] = med;
    host_res[2 * e] = (double)(cnt > 0 ? cnt : 0);
    host_res[2 * e + 1] = ok ? med : -1.0;   // -1: rank outside the bracket -> the host falls back to the full select
    if (e == 0) host_res[2 * E] = armed;
    write_a_scale(ok ? cnt : 0, med, e, a_dev, a_host);
  }
  // leave the two counters zeroed for the next round's bracket pass (no memset in the steady-state launch sequence)
  __syncthreads();
  if (threadIdx.x == 0) { cnt_lt[e] = 0u; cnt_mid[e] = 0u; }
}

}  // namespace

int launch_compact(mvicp_ctx* c, double d2_bound) {
  if (c->n_cblocks == 0) return MVICP_OK;
  double bytes = 0;
  for (int e = 0; e < c->E; ++e) if (c->owned[e]) bytes += 2.0 * 12.0 * c->frames[c->esrc[e]].n;
  // the per-edge reject masks (null table: no frame has one, and nothing is uploaded)
  const unsigned char* const* d_masks = nullptr;
  bool any_mask = false;
  for (const FrameDev& f : c->frames) if (f.grid.mask_roles) any_mask = true;
  if (any_mask) {
    std::vector<const unsigned char*> tab(2 * (size_t)c->E, nullptr);
    for (int e = 0; e < c->E; ++e) {
      tab[e] = reject_mask_of(c->frames[c->esrc[e]], MVICP_REJECT_AS_SOURCE);
      tab[c->E + e] = reject_mask_of(c->frames[c->edst[e]], MVICP_REJECT_AS_TARGET);
    }
    MV_CHECK(cached_upload(c, "mask_tab", tab.data(), sizeof(void*) * tab.size(), (void**)&d_masks));
  }
  ProfScope ps(c, "compact", bytes);
  hipLaunchKernelGGL(count_kernel, dim3(c->n_cblocks), dim3(NT), 0, c->stream, c->d_cblock_off, c->E, c->d_nsrc, c->d_cap_off, c->d_nn_idx,
                     c->d_nn_d2, d2_bound, c->d_cblock_cnt, c->d_dirty, d_masks);
  hipLaunchKernelGGL(scan_kernel, dim3(c->E), dim3(NT), 0, c->stream, c->d_cblock_off, c->d_cblock_cnt, c->d_count, c->d_dirty);
  hipLaunchKernelGGL(scatter_kernel, dim3(c->n_cblocks), dim3(NT), 0, c->stream, c->d_cblock_off, c->E, c->d_nsrc, c->d_cap_off, c->d_nn_idx,
                     c->d_nn_d2, d2_bound, c->d_cblock_cnt, c->d_first, c->d_second, c->d_cd2, c->d_qpos, c->d_dirty, d_masks);
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

// smask = omask in the frame's sorted order (f.grid.omask holds the caller's n bytes): what the acceptance test indexes
int launch_mask_permute(mvicp_ctx* c, const FrameDev& f) {
  if (f.n == 0) return MVICP_OK;
  ProfScope ps(c, "mask_permute", 5.0 * f.n);
  hipLaunchKernelGGL(mask_permute_kernel, dim3((f.n + 4 * NT - 1) / (4 * NT)), dim3(NT), 0, c->stream, f.grid.omask, f.grid.sidx, f.n, f.grid.smask);
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

int launch_gather_stream(mvicp_ctx* c) {
  if (c->n_cblocks == 0) return MVICP_OK;
  // per-edge base pointers (device table lives in the pinned staging area's device twin: small, rebuilt per call)
  std::vector<const void*> tab(3 * (size_t)c->E, nullptr);
  for (int e = 0; e < c->E; ++e) {
    tab[e] = c->frames[c->esrc[e]].grid.srec;
    tab[c->E + e] = c->frames[c->edst[e]].grid.srec;
    tab[2 * c->E + e] = c->frames[c->edst[e]].grid.snor;
  }
  const void** d_tab = nullptr;
  MV_CHECK(cached_upload(c, "gather_tab", tab.data(), sizeof(void*) * tab.size(), (void**)&d_tab));
  {
    ProfScope ps(c, "gather", 0.0);
    hipLaunchKernelGGL(gather_kernel, dim3(c->n_cblocks), dim3(NT), 0, c->stream, c->d_cblock_off, c->E, c->d_count, c->d_cap_off, c->total_cap,
                       c->d_first, c->d_second, (const PointRec* const*)d_tab, (const PointRec* const*)(d_tab + c->E), (const double* const*)(d_tab + 2 * c->E), c->d_stream, c->d_dirty);
  }
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

// cnt_lt [E] | cnt_mid [E] | hist [E][2048]; zeroed once (mvicp_set_graph, or here after a failed search), kept zero by the kernels
static int select_scratch(mvicp_ctx* c, unsigned int** cnt_lt, unsigned int** cnt_mid, unsigned int** hist) {
  const size_t E = (size_t)c->E;
  *cnt_lt = c->d_sel_hist; *cnt_mid = *cnt_lt + E; *hist = *cnt_mid + E;
  if (!c->sel_scratch_clean) {
    MV_HIP(hipMemsetAsync(c->d_sel_hist, 0, sizeof(unsigned int) * E * (kSelBins + 2), c->stream));
    c->sel_scratch_clean = true;   // (a search that does not return OK clears it again)
  }
  return MVICP_OK;
}

static void launch_bracket_final(mvicp_ctx* c, unsigned int* cnt_lt, unsigned int* cnt_mid) {
  hipLaunchKernelGGL(bracket_final_kernel, dim3(c->E), dim3(NT), 0, c->stream, c->E, c->d_count, c->d_cap_off, c->d_sel_keys1, cnt_lt,
                     cnt_mid, c->d_median, c->d_res_target ? c->d_res_target : c->d_res_host, c->spec_arm ? c->d_a : (double*)nullptr,
                     c->spec_arm ? c->d_a_check : (double*)nullptr, c->spec_arm ? 1.0 : 0.0);
}

int launch_select_bracket(mvicp_ctx* c) {
  if (c->E == 0) return MVICP_OK;
  double bytes = 0;
  for (int e = 0; e < c->E; ++e) if (c->owned[e]) bytes += 8.0 * c->hist.h_count[e];   // one full read of the key list
  ProfScope ps(c, "select", bytes);
  unsigned int *cnt_lt, *cnt_mid, *hist;
  MV_CHECK(select_scratch(c, &cnt_lt, &cnt_mid, &hist));
  if (c->n_sblocks)
    hipLaunchKernelGGL(bracket_pass_kernel, dim3(c->n_sblocks), dim3(NT), 0, c->stream, c->d_sblock_off, c->E, c->d_count, c->d_cap_off, c->d_cd2,
                       (const double*)c->d_sel_lohi, cnt_lt, c->d_sel_keys1, cnt_mid);
  launch_bracket_final(c, cnt_lt, cnt_mid);
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

int launch_select_median(mvicp_ctx* c, double d2_bound) {
  if (c->E == 0) return MVICP_OK;
  double bytes = 0;
  for (int e = 0; e < c->E; ++e) if (c->owned[e]) bytes += 16.0 * c->hist.h_count[e];   // two full reads of the key list (last round's length)
  ProfScope ps(c, "select", bytes);
  unsigned int *cnt_lt, *cnt_mid, *hist;
  MV_CHECK(select_scratch(c, &cnt_lt, &cnt_mid, &hist));
  if (c->n_sblocks) {
    long long kb;
    std::memcpy(&kb, &d2_bound, sizeof(kb));
    const long long kbq = kb > 0 ? kb >> kSelShift : 0;   // (a bound that is not a positive number anchors at 0: still monotone)
    const dim3 grid(c->n_sblocks), blk(NT);
    // (d_sel_lohi: the control-block upload of this search, which carries the host-predicted brackets, is earlier in the stream)
    hipLaunchKernelGGL(select_hist_kernel, grid, blk, 0, c->stream, c->d_sblock_off, c->E, c->d_count, c->d_cap_off, c->d_cd2, kbq, hist);
    hipLaunchKernelGGL(select_pick_kernel, dim3(c->E), blk, 0, c->stream, c->E, c->d_count, hist, kbq, c->d_sel_lohi);
    hipLaunchKernelGGL(bracket_pass_kernel, grid, blk, 0, c->stream, c->d_sblock_off, c->E, c->d_count, c->d_cap_off, c->d_cd2,
                       (const double*)c->d_sel_lohi, cnt_lt, c->d_sel_keys1, cnt_mid);
  }
  launch_bracket_final(c, cnt_lt, cnt_mid);
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

}  // namespace mvicp
