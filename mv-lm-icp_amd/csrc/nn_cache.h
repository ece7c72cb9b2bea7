// The temporal-cache rule of the exact NN kernels (nn_grid_kernel, nn_cell_kernel, nn_tile_kernel, nn_mfma_kernel).
//
// Last search left, per query, its neighbour and a lower bound L on the distance to every OTHER target (out_lb, fp32 rounded down).  Since
// then the query moved by at most eps = |dM p + dv| (1 + 1e-9) + allowance (pose update; the edge's kEdgeXf block carries dM, dv and the rounding
// allowance of search_plan.h:cache_allowance_xf, which bounds what separates that figure from the distance between the two ROUNDED queries), so every
// other target is still >= L - eps away: if the re-evaluated distance to the old neighbour is strictly below that, it is still the unique
// nearest neighbour and its exact squared distance (reference arithmetic) is the answer — no search.
#pragma once
#include "common.h"
#include "nn_list.h"

namespace mvicp {

// how far THIS query (source point p) moved since the last search, at most: |dM p + dv| plus the rounding allowance sxf[kXfCache] >= 0; the factor
// 1 + 1e-9 covers the roundings of the norm itself, which are relative to it (those of dM p + dv are not: they are in the allowance).
// 0 only when the host found the edge's query transform bit-identical to last search's (allowance 0, dM = dv = 0).
__device__ __forceinline__ double cache_eps(const double* sxf, double p0, double p1, double p2) {
  const double e0 = sxf[kXfDM] * p0 + sxf[kXfDM + 3] * p1 + sxf[kXfDM + 6] * p2 + sxf[kXfDv];
  const double e1 = sxf[kXfDM + 1] * p0 + sxf[kXfDM + 4] * p1 + sxf[kXfDM + 7] * p2 + sxf[kXfDv + 1];
  const double e2 = sxf[kXfDM + 2] * p0 + sxf[kXfDM + 5] * p1 + sxf[kXfDM + 8] * p2 + sxf[kXfDv + 2];
  return sqrt(e0 * e0 + e1 * e1 + e2 * e2) * (1.0 + 1e-9) + sxf[kXfCache];
}

// Is the query answered without a search?  lb_old = last search's bound, d = exact squared distance to the old neighbour now.
//  * same_query_hits (every kernel but nn_cell_kernel): eps == 0 — the same query bit for bit keeps last search's exact answer, whatever its
//    bound (nn_cell_kernel has no such shortcut: api.cpp's nothing_can_change relies on it);
//  * the old neighbour is provably still nearest (relative 1e-12 covers the sqrt rounding);
//  * reject_cache: the query is provably still REJECTED — its old neighbour is beyond the cutoff now (exact) and every other target was at
//    least lb_old away, i.e. is at least lb_old - eps away now: if that is beyond the cutoff too, no target is inside it, which is all the
//    reference's filter (frame.cpp:156) asks; the exact neighbour of a rejected query is never output.  out_d2 then holds the distance to the
//    OLD neighbour (>= bound: the query stays rejected downstream), out_idx keeps it as a seed, the bound is carried on.
__device__ __forceinline__ bool cache_hit(double eps, float lb_old, double d, double bound, bool same_query_hits, bool reject_cache) {
  const double nlb = (double)lb_old - eps;
  const bool still_rejected = eps != 0.0 && d >= bound && nlb > sqrt(bound) * (1.0 + 1e-9);
  return (same_query_hits && eps == 0.0) || sqrt(d) * (1.0 + 1e-12) < nlb || (reject_cache && still_rejected);
}

// No neighbour at all last time (out_lb == -1: no target within the search radius) and a bit-identical query transform (allowance 0: dM = dv
// = 0): the same query has the same answer — nothing to search, nothing to write.
__device__ __forceinline__ bool cache_still_none(double allowance, const float* out_lb, int i) { return allowance == 0.0 && out_lb[i] == -1.f; }

// What a hit leaves behind (Job = GridJob / TileJob): the exact distance, the bound carried on, the list entry.  eps == 0: bit-identical query
// transform, everything stored is already exact — nothing to write.
template <typename Job>
__device__ __forceinline__ void cache_refresh(const Job& job, int i, int pi, double d, double eps, float lb_old, double bound) {
  if (eps != 0.0) {
    job.out_d2[i] = d;
    job.out_lb[i] = __double2float_rd((double)lb_old - eps);
    if (job.list.dirty) update_list_entry(job.list, i, pi, d, bound, true);
  }
}

}  // namespace mvicp
