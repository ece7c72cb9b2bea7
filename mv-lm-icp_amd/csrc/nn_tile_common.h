// Shared pieces of the two wave-cooperative exact 1-NN kernels (nn_tile.hip: fp32 VALU screen of LDS-staged tiles; nn_mfma.hip: the
// same traversal with the screen of an opened tile on the matrix pipe): target / job views, the DPP wave reductions, the wave prologue and
// epilogue (query load, temporal-cache prologue, patch box, result store, hit census), the per-edge job table and the host side of a launch.  Everything here has internal linkage (one copy
// per translation unit, like the kernels that use it).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "nn_cache.h"
#include "nn_census.h"
#include "nn_list.h"
#include "nn_metric.h"
#include "nn_tie.h"

namespace mvicp {

namespace {

constexpr int NT = 256;
#ifndef MVICP_TILE_LEAF
#define MVICP_TILE_LEAF 32
#endif
constexpr int LEAF = MVICP_TILE_LEAF;   // points per leaf tile (tuning builds may override; 32 measured best)
constexpr int FAN = 64;    // children per node = one box per lane


// matrix-pipe operands of one cloud (nn_mfma.hip, build_mfma): per tile 64 x 16 B — lane l's A fragment of v_mfma_f32_32x32x16_f16 for
// the tile's point l & 31 — and per block (= 64 tiles = one level-0 node) the origin / scale / error terms those fragments refer to
struct MfBlock { double cx, cy, cz, scale; float db, en, pad0, pad1; };

struct TileView {
  const double* spts; const int* sidx; int n;
  const float* wide; int levels;  // number of box levels (>= 1)
  int cnt[6]; long long off[6];
  double maxabs;                  // largest |coordinate| in the cloud
  const PointRec* srec;           // sorted 32-B records {x, y, z, original index}
  const uint4* mf_ops; const MfBlock* mf_blk;
};

struct TileJob {
  TileView dst;
  const double* q; const int* qidx; const double* xf; int n;
  int* out_idx; double* out_d2;
  const int* inv;   // target original index -> sorted position
  int seed;         // out_idx still holds last round's neighbours (sorted positions, -1 = none): use them as starting candidates
  float* out_lb;    // BND builds (fp32, rounded down): per query, a lower bound on the distance to every target other than out_idx (the grid kernel's temporal cache)
  float mu;         // BND builds: width of the extra guard band (metres) that makes that bound useful
  // BND builds, cache-aware rounds (round 3): out_lb holds last search's bounds and the edge's query transform carries the temporal-cache
  // allowance (xf[kXfCache] >= 0): a lane whose neighbour provably did not change sits the traversal out, like in nn_grid_kernel.  `list`
  // (list.dirty != null) = the edge's compacted list is maintained in place by this launch (nn_list.h).
  int cache;
  int reject_cache; // cache-aware rounds: a query that is provably still rejected by the cutoff (old neighbour and every other target beyond it) is a hit too
  int miss_max;     // cache-aware rounds of nn_tile_kernel: a wave with at most this many missed lanes answers them one by one (miss_block); 0 = off
  ListRef list;
  float kacc; int trig;   // nn_mfma.hip tunables (ctx::mfma_kacc, mfma_trig)
  TieRef tie;             // where lanes whose best distance was met by more than one target report (nn_tie.h)
};

// Wave-wide reductions on the DPP network (row quad-perm / mirror steps, then row_bcast15 / row_bcast31; lane 63 ends up with the
// result, broadcast through readlane -> SGPRs).  __shfl_xor would go through ds_bpermute: ~12 LDS-crossbar round trips per reduction,
// and this kernel reduces once per traversal step.
// fp32 reductions of NON-NEGATIVE values (incl. +inf): their bit patterns order like unsigned integers, so the whole
// reduction is six v_min_u32 / v_max_u32 with the DPP permutation fused into the operand (the builtin form costs a
// mov + mov_dpp + op per step).  "s_nop 1": a VALU result needs two wait states before a DPP read of it.
#define MVICP_DPP_CHAIN(OP)                                                         \
  "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
  "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
  "s_nop 1\n\t" OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"          \
  "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"        \
  "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"        \
  "s_nop 1"
__device__ __forceinline__ float wave_max_f(float nonneg) {
  unsigned int v = (unsigned int)__float_as_int(nonneg);
  asm volatile(MVICP_DPP_CHAIN("v_max_u32_dpp") : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane((int)v, 63));
}
__device__ __forceinline__ float wave_min_f(float nonneg) {
  unsigned int v = (unsigned int)__float_as_int(nonneg);
  asm volatile(MVICP_DPP_CHAIN("v_min_u32_dpp") : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane((int)v, 63));
}
// fp32 reductions of ARBITRARY floats (negative coordinates, +-inf): the key  b ^ ((b >> 31) & 0x7fffffff)  orders like the float as a
// signed integer and is its own inverse, so the wave minimum / maximum is again six DPP-fused v_min_i32 / v_max_i32.
__device__ __forceinline__ int fkey(float f) { const int b = __float_as_int(f); return b ^ ((b >> 31) & 0x7fffffff); }
__device__ __forceinline__ float wave_min_any(float f) {
  int v = fkey(f);
  asm volatile(MVICP_DPP_CHAIN("v_min_i32_dpp") : "+v"(v));
  return __int_as_float(fkey(__int_as_float(__builtin_amdgcn_readlane(v, 63))));
}
__device__ __forceinline__ float wave_max_any(float f) {
  int v = fkey(f);
  asm volatile(MVICP_DPP_CHAIN("v_max_i32_dpp") : "+v"(v));
  return __int_as_float(fkey(__int_as_float(__builtin_amdgcn_readlane(v, 63))));
}
__device__ __forceinline__ float bcast(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}


// screen threshold for a running best: (sqrt(best) + slack)^2 with 2^-20 relative head-room
__device__ __forceinline__ float thr_of(double best, float slack) {
  const float rb = (float)sqrt(best) * 1.000001f + slack;
  return rb * rb * 1.000002f;
}

// ---- the wave prologue and epilogue of nn_tile_kernel / nn_mfma_kernel (LaneT = Lane / LaneM; WG = threads per workgroup) ----

// query load and transform (frame.cpp:117-118,131,136); p = the source point, what the temporal cache measures the displacement of
template <typename LaneT>
__device__ __forceinline__ void load_query(const TileJob& job, const double* sxf, bool has_xf, int i, LaneT& L, double& p0, double& p1, double& p2) {
  if (L.active) {
    p0 = job.q[3 * (size_t)i]; p1 = job.q[3 * (size_t)i + 1]; p2 = job.q[3 * (size_t)i + 2];
    if (has_xf) xf_point(sxf, p0, p1, p2, L.qx, L.qy, L.qz);
    else { L.qx = p0; L.qy = p1; L.qz = p2; }
  }
}

// Temporal cache (BND builds in cache-aware rounds; nn_cache.h, the same test as nn_grid_kernel's plus the still-rejected clause): seed_pi /
// seed_d = last round's neighbour and the re-evaluated distance to it.  A lane whose neighbour provably did not change is finished here and
// sits the traversal out: the wave walks the hierarchy for its MISSED lanes only — a patch of a few queries opens one or two tiles instead of
// six.  The still-rejected lanes are the ones with the LARGEST balls (their thresholds reach the search radius): taking them out of the
// traversal is what makes a partial-overlap round cheap.
template <bool BND>
__device__ __forceinline__ void cache_prologue(const TileJob& job, const double* sxf, bool has_xf, int i, double p0, double p1, double p2, int seed_pi, double seed_d,
                                               double bound, bool& active, unsigned int& n_hit) {
  if (BND && job.cache && has_xf && job.seed && active && seed_pi < 0 && cache_still_none(sxf[kXfCache], job.out_lb, i)) {
    active = false;
    n_hit = 1;
  }
  if (BND && job.cache && has_xf && seed_pi >= 0) {
    if (sxf[kXfCache] >= 0.0) {
      const double eps = cache_eps(sxf, p0, p1, p2);
      const float lb_old = job.out_lb[i];
      if (cache_hit(eps, lb_old, seed_d, bound, true, job.reject_cache)) {
        cache_refresh(job, i, seed_pi, seed_d, eps, lb_old, bound);
        active = false;
        n_hit = 1;
      }
    }
  }
}

// census (profiling only): the wave's slot, and its count of lanes answered by the cache
template <int WG>
__device__ __forceinline__ size_t census_slot() { return ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (WG / 64) + (threadIdx.x >> 6); }
template <int WG>
__device__ __forceinline__ void census_hits(unsigned long long* stats, unsigned int n_hit) {
  const unsigned long long hits = __popcll(__ballot(n_hit != 0u));
  if ((threadIdx.x & 63) == 0) stats[8 * census_slot<WG>() + 3] = hits;
}

// a wave without a miss leaves at once: true = all 64 lanes were answered by the cache
template <bool BND, int WG>
__device__ __forceinline__ bool cache_all_hit(const TileJob& job, bool active, unsigned int n_hit, unsigned long long* stats) {
  if (BND && job.cache && __ballot(active) == 0ull) {
    if (stats) census_hits<WG>(stats, n_hit);
    return true;
  }
  return false;
}

struct PatchBox {      // wave-uniform patch description (lives in SGPRs)
  float lo[3], hi[3], c[3];   // the patch AABB in fp32, rounded OUTWARD, and its centre (the coarse cull runs in fp32)
  float slack;         // fp32 screening guard band (metres)
  float mu;            // BND builds: extra guard band (0 otherwise)
};

// patch box in fp32, rounded outward: min / max of the lanes' float copies, widened by more than the half ulp a conversion can have moved a
// coordinate inwards (six DPP reductions of 7 instructions; round 2 reduced the fp64 coordinates: ~30 instructions each).  Returns the largest
// coordinate magnitude either operand of a difference can have: the cloud's box and the patch.
template <bool BND, typename LaneT>
__device__ __forceinline__ float patch_box(const TileJob& job, const LaneT& L, PatchBox& G) {
  const float inf = __int_as_float(0x7f800000);
  const float a = (float)L.qx, b = (float)L.qy, c2 = (float)L.qz;
  float lo[3] = {wave_min_any(L.active ? a : inf), wave_min_any(L.active ? b : inf), wave_min_any(L.active ? c2 : inf)};
  float hi[3] = {wave_max_any(L.active ? a : -inf), wave_max_any(L.active ? b : -inf), wave_max_any(L.active ? c2 : -inf)};
  float m = (float)job.dst.maxabs * 1.000001f;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    lo[ax] -= fabsf(lo[ax]) * 1.2e-7f + 1e-37f; hi[ax] += fabsf(hi[ax]) * 1.2e-7f + 1e-37f;
    G.lo[ax] = lo[ax]; G.hi[ax] = hi[ax]; G.c[ax] = 0.5f * (lo[ax] + hi[ax]);
    m = fmaxf(m, fmaxf(fabsf(lo[ax]), fabsf(hi[ax])));
  }
  // per axis: |fl32(q) - q| + |fl32(p) - p| + rounding of the fp32 subtraction <= 3 * 2^-24 * m; x sqrt(3) axes, x2 safety
  G.slack = m * (3.0f * 1.7320508f * 2.0f / 16777216.0f) * 1.00001f + 1e-30f;
  G.mu = BND ? job.mu : 0.f;
  return m;
}

// ---- the node prologue of both kernels' visit<LEVEL> ----
// Register budget: the traversal recurses (level 2 -> 1 -> 0 -> tile scan) and everything a level keeps across the descent is live in all
// deeper levels.  Levels 1 and 2 therefore park their 64 child boxes in wave-private LDS (32 B each, read back with one uniform-address load
// per step) and keep only {cull distance, order key, pending} per lane; level 0 keeps its boxes in registers and broadcasts them (v_readlane).
struct NodeBoxes { float b0, b1, b2, b3, b4, b5; };   // one child box per lane: lo.xyz, hi.xyz (inverted = empty beyond nchild)

template <int LEVEL>
__device__ __forceinline__ NodeBoxes node_fetch(const TileView& g, int first, int nchild) {
  const int lane = threadIdx.x & 63;
  const float inf = __int_as_float(0x7f800000);
  float b0 = inf, b1 = inf, b2 = inf, b3 = -inf, b4 = -inf, b5 = -inf;
  if (lane < nchild) {
    const float* base = g.wide + g.off[LEVEL] + first + lane;
    const long long st = g.cnt[LEVEL];
    b0 = base[0]; b1 = base[st]; b2 = base[2 * st]; b3 = base[3 * st]; b4 = base[4 * st]; b5 = base[5 * st];
  }
  return NodeBoxes{b0, b1, b2, b3, b4, b5};
}

// coarse cull: child box vs the patch AABB; valid for every lane because lb_lane >= box-box distance.  fp32 against the outward-rounded patch
// box: every operation rounds by <= 2^-24 relative, (1 - 1e-6) more than covers the five of them, so ddf stays a lower bound of the
// box-to-patch distance (round 3: was fp64 — 12 conversions + ~20 fp64 operations per node).  key: visiting order only.
__device__ __forceinline__ void node_cull(const PatchBox& G, const NodeBoxes& B, float& ddf, float& key) {
  const float e0 = fmaxf(fmaxf(B.b0 - G.hi[0], G.lo[0] - B.b3), 0.f);
  const float e1 = fmaxf(fmaxf(B.b1 - G.hi[1], G.lo[1] - B.b4), 0.f);
  const float e2 = fmaxf(fmaxf(B.b2 - G.hi[2], G.lo[2] - B.b5), 0.f);
  ddf = (e0 * e0 + e1 * e1 + e2 * e2) * 0.999999f;
  const float k0 = fmaxf(fmaxf(B.b0 - G.c[0], G.c[0] - B.b3), 0.f);
  const float k1 = fmaxf(fmaxf(B.b1 - G.c[1], G.c[1] - B.b4), 0.f);
  const float k2 = fmaxf(fmaxf(B.b2 - G.c[2], G.c[2] - B.b5), 0.f);
  key = k0 * k0 + k1 * k1 + k2 * k2;
}

// levels 1 and 2: park the boxes in the level's third of the wave's LDS ([axis][child] -> (lo, hi))
__device__ __forceinline__ void node_park(float2* __restrict__ mybox, const NodeBoxes& B) {
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_wave_barrier();
  mybox[lane] = make_float2(B.b0, B.b3);
  mybox[FAN + lane] = make_float2(B.b1, B.b4);
  mybox[2 * FAN + lane] = make_float2(B.b2, B.b5);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// child c's box for every lane: read back from LDS, or broadcast from lane c's registers
template <bool IN_LDS>
__device__ __forceinline__ NodeBoxes node_child(const float2* __restrict__ mybox, const NodeBoxes& B, int c) {
  if (IN_LDS) {
    const float2 u = mybox[c], v = mybox[FAN + c], w = mybox[2 * FAN + c];
    return NodeBoxes{u.x, v.x, w.x, u.y, v.y, w.y};
  }
  return NodeBoxes{bcast(B.b0, c), bcast(B.b1, c), bcast(B.b2, c), bcast(B.b3, c), bcast(B.b4, c), bcast(B.b5, c)};
}

// An answered lane's results, in the sorted order of the source cloud.  The neighbour is `key`: its sorted position (-1: none inside the cutoff),
// or with BY_INDEX its original index (0x7fffffff: none), mapped to the position through job.inv.
template <bool BND, bool BY_INDEX>
__device__ __forceinline__ void store_result(const TileJob& job, int i, int key, double best, double second, bool tie, float mu, double bound) {
  constexpr int NONE = BY_INDEX ? 0x7fffffff : -1;
  job.out_idx[i] = key == NONE ? -1 : (BY_INDEX && job.inv ? job.inv[key] : key);
  job.out_d2[i] = best;
  if (BND) job.out_lb[i] = key == NONE ? -1.f : __double2float_rd(fmin(sqrt(second), sqrt(best) + (double)mu) * (1.0 - 1e-9));
  if (job.list.dirty) update_list_entry(job.list, i, key == NONE ? -1 : (BY_INDEX ? job.inv[key] : key), best, bound, false);
  if ((BND ? second == best : tie) && key != NONE) tie_report(job.tie, (unsigned int)i);
}
TileView view_of(const FrameDev& f) {
  TileView v;
  v.spts = f.grid.spts; v.sidx = f.grid.sidx; v.n = f.n;
  v.wide = f.grid.wide; v.levels = f.grid.wide_levels;
  for (int l = 0; l < 6; ++l) { v.cnt[l] = f.grid.wide_cnt[l]; v.off[l] = f.grid.wide_off[l]; }
  v.maxabs = f.grid.maxabs;
  v.srec = (const PointRec*)f.grid.srec;
  v.mf_ops = (const uint4*)f.grid.mf_ops; v.mf_blk = (const MfBlock*)f.grid.mf_blk;
  return v;
}

// the per-edge job table of a launch (one TileJob per active edge of this rank)
inline int build_tile_jobs(mvicp_ctx* c, bool with_bounds, bool with_cache, bool with_list, std::vector<TileJob>& jobs, int& max_n, double& nq, std::vector<TieJob>& ties) {
  max_n = 0; nq = 0;
  double launch_q = 0;
  for (int e = 0; e < c->E; ++e) if (c->active[e]) launch_q += c->frames[c->esrc[e]].n;
  const TieRef tref = tie_ref(c, (size_t)launch_q, 0u);
  for (int e = 0; e < c->E; ++e) {
    if (!c->active[e]) continue;
    const FrameDev& s = c->frames[c->esrc[e]];
    const FrameDev& d = c->frames[c->edst[e]];
    if (!s.has_grid || !d.has_grid) { set_error("tile NN needs the per-cloud structure on frames %d and %d", c->esrc[e], c->edst[e]); return MVICP_ERR_STATE; }
    TileJob j;
    std::memset(&j, 0, sizeof(j));  // padding too: the table is cached by content
    j.dst = view_of(d);
    j.q = s.grid.spts; j.qidx = nullptr; j.xf = c->d_xf + (size_t)e * kEdgeXf; j.n = s.n;
    j.out_idx = c->d_nn_idx + c->cap_off[e]; j.out_d2 = c->d_nn_d2 + c->cap_off[e];
    j.inv = d.grid.inv;
    j.seed = (c->tile_seed && (int)c->hist.nn_cache_edge.size() == c->E && c->hist.nn_cache_edge[e]) ? 1 : 0;
    if (with_bounds) { j.out_lb = c->d_nn_lb + c->cap_off[e]; j.mu = (float)(c->opt.tile_mu * d.grid.cell); }
    if (with_bounds && with_cache) { j.cache = 1; j.miss_max = c->tile_miss; j.reject_cache = c->reject_cache ? 1 : 0; }
    if (with_list) {
      j.list = ListRef{c->d_qpos + c->cap_off[e], c->d_second + c->cap_off[e], c->d_cd2 + c->cap_off[e], c->d_dirty + e, c->d_dirty_slots + c->dslot_off[e],
                       c->d_stream + c->cap_off[e], c->total_cap, d.grid.snor, (const PointRec*)d.grid.srec,
                       reject_mask_of(s, MVICP_REJECT_AS_SOURCE), reject_mask_of(d, MVICP_REJECT_AS_TARGET)};
    }
    j.kacc = (float)c->mfma_kacc; j.trig = c->mfma_trig;
    j.tie = tref; j.tie.job = (unsigned int)jobs.size();
    {
      TieJob t;
      std::memset(&t, 0, sizeof(t));
      tie_job_fill(d, t);
      t.q = j.q; t.xf = j.xf; t.n = j.n; t.out_idx = j.out_idx; t.out_d2 = j.out_d2; t.inv = j.inv; t.list = j.list;
      ties.push_back(t);
    }
    jobs.push_back(j);
    max_n = std::max(max_n, s.n);
    nq += s.n;
  }
  return MVICP_OK;
}

// Everything a launch of either kernel shares on the host: job table, cached upload, census scratch, tie fix-up, dirty reduce, census collect.
// wg = threads per workgroup, scope = profile scope, launch(jobs, d_jobs, grid, top, d_stats) = the kernel selection (top >= 0: every target
// has top + 1 hierarchy levels, -1: mixed).
template <typename Launch>
inline int launch_tile_search(mvicp_ctx* c, double d2_bound, bool with_bounds, bool with_cache, bool with_list, int wg, const char* scope, Launch launch) {
  std::vector<TileJob> jobs;
  int max_n = 0;
  double nq = 0;
  std::vector<TieJob> ties;
  MV_CHECK(build_tile_jobs(c, with_bounds, with_cache, with_list, jobs, max_n, nq, ties));
  if (jobs.empty() || max_n == 0) return MVICP_OK;
  TileJob* d_jobs = nullptr;
  MV_CHECK(cached_upload(c, jobs[0].xf ? "tile_jobs" : "tile_jobs_raw", jobs.data(), sizeof(TileJob) * jobs.size(), (void**)&d_jobs));
  unsigned long long* d_stats = nullptr;
  const size_t slots = (size_t)((max_n + wg - 1) / wg) * jobs.size() * (wg / 64);
  MV_CHECK(census_scratch(c, slots, &d_stats));
  {
    ProfScope ps(c, scope, 36.0 * nq);  // query read 24 B + result write 12 B; candidate / tile-operand / box bytes come from the census
    const dim3 grid((max_n + wg - 1) / wg, (unsigned)jobs.size());
    int top = jobs[0].dst.levels - 1;   // same depth everywhere -> the traversal specialised for it
    for (const TileJob& j : jobs) if (j.dst.levels - 1 != top) top = -1;
    launch(jobs, d_jobs, grid, top, d_stats);
  }
  MV_HIP(hipGetLastError());
  MV_CHECK(launch_tie_fixup(c, ties, d2_bound));     // exact distance ties: the reference's own descent decides (nn_tie.hip); before the lists are read
  if (with_list) MV_CHECK(launch_dirty_reduce(c));   // per-edge OR of the "list membership changed" slots
  if (d_stats) MV_CHECK(census_collect(c, d_stats, slots, nq, 2, scope));
  return MVICP_OK;
}

}  // namespace

}  // namespace mvicp
