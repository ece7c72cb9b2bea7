// Overlap census (mvicp_overlap): for every ordered pair of clouds (i, j) at the given poses, how many sample points of cloud i
// have a point of cloud j within the cutoff, and the exact integer sum of their scaled squared distances.  DESIGN.md §3.6.
//
// One persistent launch over all pairs.  A work item is `item` (8 .. 256, chosen by the host from the size of the census) consecutive
// samples of ONE pair and belongs to one wave, so the reduction needs no segmented logic: two integer atomics per item.  The descents
// are chains of dependent memory round trips (a query at the noisy initial poses opens tens of leaves), so what a small census needs is
// as many of them in flight as the chip holds — items of 8 samples, one per octet — while a large one amortises the per-item work over
// 256 samples.  Per 64 samples:
//   (A) one sample per lane: transform it (the rounded operations of mvicp_correspond's query transform, nn_metric.h) and test it
//       against the target's ROOT box — a lower bound at or beyond the cutoff is a miss without any descent, which is what makes the
//       pairs that do not overlap (most of K^2) nearly free;
//   (B) the survivors, eight at a time, one per lane octet: bounded exact 1-NN DISTANCE in the target's implicit 8-ary box tree
//       (the structure and the octet descent of nn_far_kernel, nn_grid.hip).  The descent starts at best = B2 (nothing at or beyond
//       the cutoff needs resolving), prunes with lb >= best — only the minimum leaves the kernel, so a box that can at most tie it is
//       not opened: no index, no tie order, no second best, no bounds for a cache — and scans leaves eight points per step.
// Exactness: lb is evaluated in the same rounded, monotone operations as dist2 on a box rounded outward, so lb <= d2 for every point
// in the box; a pruned box holds no point below the running minimum, and min d2 is therefore the brute-force minimum whenever that
// is < B2.  hits / sumq are integer sums: independent of the order of the atomics.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "nn_metric.h"

namespace mvicp {

namespace {

constexpr int NT = 256;     // threads per workgroup: 4 waves, 32 octets
constexpr int ITEM_MAX = 256, ITEM_MIN = 8;   // samples per work item (a power of two, chosen per launch)

struct alignas(16) OvJob {
  double xf[kXfRigid];            // Rs ts Rd^-1 td of the pair (the rigid part of an edge's kEdgeXf)
  const double* q;                // source cloud, sorted order (n x 3)
  const int* samp;                // sorted positions of the samples, ascending (null: every point, position t)
  const double* tpts;             // target cloud, sorted order
  const float* oct;               // its implicit 8-ary box tree (node 0 = root box)
  long long first_leaf;
  int s, tn, oct_leaf, pair;      // samples of the source, points of the target, points per leaf, i * K + j
};
static_assert(sizeof(OvJob) == 256, "OvJob layout");

__global__ __launch_bounds__(NT) void overlap_kernel(const OvJob* __restrict__ jobs, const long long* __restrict__ item_off, int n_jobs, long long n_items,
                                                     int item_size, int top_stride, double B2, double scale, int* __restrict__ hits,
                                                     unsigned long long* __restrict__ sumq) {
  __shared__ int s_id[NT / 8][OCT_STACK];
  __shared__ double s_lb[NT / 8][OCT_STACK];
  const int lane = threadIdx.x & 63, l = lane & 7, o = lane >> 3, obase = lane & ~7;
  const int oct = threadIdx.x >> 3;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long n_waves = (long long)gridDim.x * (NT / 64);
  for (long long item = (long long)blockIdx.x * (NT / 64) + wave; item < n_items; item += n_waves) {
    // the job whose item range holds `item`: a 64-ary search, one job offset per lane and level (item_off is strictly increasing and
    // item_off[0] = 0 <= item, so the lanes that say yes are a non-empty prefix)
    int jb = 0;
    for (int stride = top_stride; stride >= 1; stride >>= 6) {
      const long long idx = (long long)jb + (long long)lane * stride;
      const bool le = idx < n_jobs && item_off[idx] <= item;
      jb += (__popcll(__ballot(le)) - 1) * stride;
    }
    const int jlo = __builtin_amdgcn_readfirstlane(jb);
    const OvJob& J = jobs[jlo];
    const long long t0 = (item - item_off[jlo]) * item_size;
    const int t1 = (int)min(t0 + item_size, (long long)J.s);
    const long long first_leaf = J.first_leaf;
    const int per_leaf = J.oct_leaf, tn = J.tn;
    const double* __restrict__ tp = J.tpts;
    const float* __restrict__ tree = J.oct;
    int h = 0;
    unsigned long long sq = 0;   // (both live in lane 0 of every octet)
    for (int tb = (int)t0; tb < t1; tb += 64) {
      // (A) one sample per lane: transform + root-box test
      const int t = tb + lane;
      double qx = 0.0, qy = 0.0, qz = 0.0;
      bool alive = false;
      if (t < t1) {
        const size_t pos = J.samp ? (size_t)J.samp[t] : (size_t)t;
        const double p0 = J.q[3 * pos], p1 = J.q[3 * pos + 1], p2 = J.q[3 * pos + 2];
        xf_point(J.xf, p0, p1, p2, qx, qy, qz);
        const float4* rb = reinterpret_cast<const float4*>(tree);
        alive = oct_box_lb(qx, qy, qz, rb[0], rb[1]) < B2;
      }
      unsigned long long mask = __ballot(alive);
      // (B) eight survivors at a time, one per octet
      while (mask) {
        unsigned long long m = mask;
#pragma unroll
        for (int k = 0; k < 7; ++k) if (k < o) m &= m - 1;   // octet o takes the o-th survivor
        const int src = m ? __ffsll((long long)m) - 1 : -1;
        const int from = src < 0 ? lane : src;
        const double ox = __shfl(qx, from, 64), oy = __shfl(qy, from, 64), oz = __shfl(qz, from, 64);
#pragma unroll
        for (int k = 0; k < 8; ++k) mask &= mask - 1;
        if (src < 0) continue;
        double best = B2;
        if (l == 0) { s_id[oct][0] = 0; s_lb[oct][0] = 0.0; }
        int sp = 1;
        while (sp > 0) {
          --sp;
          const int id = s_id[oct][sp];
          if (s_lb[oct][sp] >= best) continue;
          if (id >= first_leaf) {
            const long long j = (long long)id - first_leaf;
            const int lo = (int)min(j * per_leaf, (long long)tn), hi = min(lo + per_leaf, tn);
            // 32 points per step: four per lane, loaded together (a lane past the end re-reads the leaf's last point)
            double d = best;
            for (int b = lo; b < hi; b += 32) {
              double c[4][3];
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const size_t k = (size_t)min(b + l + 8 * u, hi - 1);
                c[u][0] = tp[3 * k]; c[u][1] = tp[3 * k + 1]; c[u][2] = tp[3 * k + 2];
              }
#pragma unroll
              for (int u = 0; u < 4; ++u) d = fmin(d, dist2(ox, oy, oz, c[u][0], c[u][1], c[u][2]));
            }
#pragma unroll
            for (int x = 1; x < 8; x <<= 1) d = fmin(d, __shfl_xor(d, x, 64));
            best = d;
            continue;
          }
          // internal node: one child box per lane (32 B each, 256 B contiguous per octet)
          const float4* bx = reinterpret_cast<const float4*>(tree + 8 * ((size_t)8 * id + 1 + l));
          const double lb = oct_box_lb(ox, oy, oz, bx[0], bx[1]);
          const bool pass = lb < best;
          int rank = 0, npass = 0;   // rank among the passing children by (lb, lane): the nearest goes on top
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const double lk = __shfl(lb, obase + k, 64);
            const bool pk = lk < best;
            npass += pk ? 1 : 0;
            rank += (pk && (lk < lb || (lk == lb && k < l))) ? 1 : 0;
          }
          if (pass) {
            const int pos = sp + (npass - 1 - rank);
            s_id[oct][pos] = 8 * id + 1 + l;
            s_lb[oct][pos] = lb;
          }
          sp += npass;
        }
        if (l == 0 && best < B2) { ++h; sq += (unsigned long long)(long long)(best * scale); }   // floor(d2 * 2^q_exp) < 2^31, exact
      }
    }
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) { h += __shfl_xor(h, x, 64); sq += __shfl_xor(sq, x, 64); }
    if (lane == 0 && h) { atomicAdd(&hits[J.pair], h); atomicAdd(&sumq[J.pair], sq); }
  }
}


// the cloud's sample list for `s` samples of its n points: positions inv[floor(t n / s)], ascending
int ensure_samples(GridDev& G, int n, int s) {
  if (s == n || (G.ov_samp && G.ov_samp_s == s)) return MVICP_OK;
  std::vector<int> pos((size_t)s);
  for (int t = 0; t < s; ++t) pos[t] = G.h_inv[(size_t)((long long)t * n / s)];
  std::sort(pos.begin(), pos.end());
  if (G.ov_samp) MV_HIP(hipFree(G.ov_samp));   // (only census kernels read it, and every census waits for its own)
  G.ov_samp = nullptr; G.ov_samp_s = 0;
  MV_HIP(hipMalloc((void**)&G.ov_samp, sizeof(int) * (size_t)s));
  MV_HIP(hipMemcpy(G.ov_samp, pos.data(), sizeof(int) * (size_t)s, hipMemcpyHostToDevice));
  G.ov_samp_s = s;
  return MVICP_OK;
}

}  // namespace

void free_overlap(mvicp_ctx* c) {
  if (c->ov_dev) (void)hipFree(c->ov_dev);
  if (c->ov_pin) (void)hipHostFree(c->ov_pin);
  c->ov_dev = nullptr; c->ov_pin = nullptr; c->ov_bytes = 0;
}

int overlap_census(mvicp_ctx* c, const double* xf, double B2, double scale, int max_samples, int* samples, int* hits, long long* sumq) {
  const int K = c->n_frames;
  const size_t KK = (size_t)K * K;
  for (int i = 0; i < K; ++i) {
    FrameDev& f = c->frames[i];
    const int s = (max_samples <= 0 || max_samples >= f.n) ? f.n : max_samples;
    samples[i] = s;
    if (f.n == 0) continue;
    if (!f.has_grid) { set_error("frame %d has no structures", i); return MVICP_ERR_STATE; }
    if (f.grid.oct_first_leaf > 299593) { set_error("frame %d: box tree deeper than the descent stack", i); return MVICP_ERR_INTERNAL; }
    MV_CHECK(ensure_samples(f.grid, f.n, s));
  }
  std::memset(hits, 0, sizeof(int) * KK);
  if (sumq) std::memset(sumq, 0, sizeof(long long) * KK);
  for (int i = 0; i < K; ++i) hits[(size_t)i * K + i] = samples[i];

  // jobs: every ordered pair with a sample and a target point
  std::vector<OvJob> jobs;
  std::vector<long long> item_off(1, 0);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) {
      const FrameDev& fs = c->frames[i];
      const FrameDev& ft = c->frames[j];
      if (i == j || samples[i] == 0 || ft.n == 0) continue;
      OvJob J;
      std::memcpy(J.xf, xf + kXfRigid * ((size_t)i * K + j), sizeof(J.xf));
      J.q = fs.grid.spts; J.samp = samples[i] == fs.n ? nullptr : fs.grid.ov_samp;
      J.tpts = ft.grid.spts; J.oct = ft.grid.oct; J.first_leaf = ft.grid.oct_first_leaf;
      J.s = samples[i]; J.tn = ft.n; J.oct_leaf = ft.grid.oct_leaf; J.pair = i * K + j;
      jobs.push_back(J);
    }
  if (jobs.empty()) return MVICP_OK;
  // resident grid: what the registers and the LDS stacks admit per CU (at most 7 by the stacks)
  int cus = 0, per_cu = 0;
  MV_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  MV_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, overlap_kernel, NT, 0));
  const long long resident = (long long)std::max(cus, 1) * std::min(std::max(per_cu, 1), 7);
  // samples per work item: small while the census has fewer items than eight per resident wave
  long long total = 0;
  for (const OvJob& J : jobs) total += J.s;
  int item_size = ITEM_MAX;
  while (item_size > ITEM_MIN && total / item_size < 8 * resident * (NT / 64)) item_size >>= 1;
  for (const OvJob& J : jobs) item_off.push_back(item_off.back() + (J.s + item_size - 1) / item_size);
  const long long n_items = item_off.back();
  int top_stride = 1;
  while ((long long)top_stride * 64 < (long long)jobs.size()) top_stride *= 64;

  // buffers of the census's own: [jobs | item offsets | hits | sumq]
  const size_t off_items = align256(sizeof(OvJob) * jobs.size()), off_hits = off_items + align256(sizeof(long long) * item_off.size());
  const size_t off_sumq = off_hits + align256(sizeof(int) * KK), bytes = off_sumq + align256(sizeof(long long) * KK);
  if (bytes > c->ov_bytes) {
    free_overlap(c);
    MV_HIP(hipMalloc((void**)&c->ov_dev, bytes));
    MV_HIP(hipHostMalloc((void**)&c->ov_pin, bytes, hipHostMallocDefault));
    c->ov_bytes = bytes;
  }
  std::memcpy(c->ov_pin, jobs.data(), sizeof(OvJob) * jobs.size());
  std::memcpy(c->ov_pin + off_items, item_off.data(), sizeof(long long) * item_off.size());
  std::memset(c->ov_pin + off_hits, 0, bytes - off_hits);
  MV_HIP(hipMemcpyAsync(c->ov_dev, c->ov_pin, bytes, hipMemcpyHostToDevice, c->stream));
  const long long want = (n_items + NT / 64 - 1) / (NT / 64);
  const int blocks = (int)std::max<long long>(1, std::min<long long>(want, resident));
  hipLaunchKernelGGL(overlap_kernel, dim3(blocks), dim3(NT), 0, c->stream, reinterpret_cast<const OvJob*>(c->ov_dev),
                     reinterpret_cast<const long long*>(c->ov_dev + off_items), (int)jobs.size(), n_items, item_size, top_stride, B2, scale,
                     reinterpret_cast<int*>(c->ov_dev + off_hits), reinterpret_cast<unsigned long long*>(c->ov_dev + off_sumq));
  MV_HIP(hipGetLastError());
  MV_HIP(hipMemcpyAsync(c->ov_pin + off_hits, c->ov_dev + off_hits, bytes - off_hits, hipMemcpyDeviceToHost, c->stream));
  MV_HIP(hipStreamSynchronize(c->stream));
  const int* gh = reinterpret_cast<const int*>(c->ov_pin + off_hits);
  const long long* gs = reinterpret_cast<const long long*>(c->ov_pin + off_sumq);
  for (const OvJob& J : jobs) {
    hits[J.pair] = gh[J.pair];
    if (sumq) sumq[J.pair] = gs[J.pair];
  }
  return MVICP_OK;
}

}  // namespace mvicp
