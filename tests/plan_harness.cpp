// Thin extern "C" layer over mv-lm-icp_amd/csrc/search_plan.h for tests/test_search_plan_cpu.py (TEST INFRASTRUCTURE, host only: no HIP, no
// GPU).  A Planner stands for what mvicp_ctx holds of a search — options, history, plan and the memory the plan is written into — and the
// functions below are the calls api.cpp makes around plan_search, with the observables of a round (counts, medians, tie / far words) fed in
// by the caller.
#include <cstring>
#include <string>
#include <vector>

#include "../mv-lm-icp_amd/csrc/search_plan.h"

using namespace mvicp;

namespace {
struct Planner {
  int E = 0, K = 0;
  std::vector<int> esrc, edst;
  std::vector<char> owned;
  std::vector<PlanFrame> frames;
  SearchOptions opt;
  SearchHistory hist;
  SearchPlan plan;
  SearchInputs in;
  // what the executor lends the plan: the masks and region 1 of the control-block mirror
  std::vector<char> active, src_fixed;
  std::vector<double> xf, lohi;
  std::vector<int> nsrc, dirty;
  std::vector<double> poses;
  std::vector<unsigned char> fixed;
};
}  // namespace

extern "C" {

// the plan of one call, flattened (tests/test_search_plan_cpu.py PlanOut mirrors it field for field)
struct PlanOut {
  int status, method, tile_lb, tile_cached, handed_over, cached_on_mfma;
  int all_same, same_active_set, all_unchanged;
  int nothing_can_change, tie_skip, far_skip, far_narrow, tie_launched, far_launched, sel_skip;
  int use_bracket, spec_arm, spec2_plan, n_tie_need;
  double eps_over_mu;
};

void* plan_new(int n_frames, int E, const int* src, const int* dst, const unsigned char* owned) {
  Planner* P = new Planner;
  P->E = E; P->K = n_frames;
  P->esrc.assign(src, src + E); P->edst.assign(dst, dst + E); P->owned.assign(owned, owned + E);
  P->frames.assign(n_frames, PlanFrame());
  P->active.assign(E, 0); P->src_fixed.assign(E, 0); P->xf.assign((size_t)E * kEdgeXf, 0.0); P->lohi.assign(2 * (size_t)E, 0.0);
  P->nsrc.assign(E, 0); P->dirty.assign(E, 0);
  P->hist.new_graph(E);   // (what mvicp_set_graph does)
  return P;
}
void plan_free(void* h) { delete (Planner*)h; }

// flags: 1 = has the grid structures, 2 = has a tie tree, 4 = has sorted normals
void plan_set_frame(void* h, int k, int n, double max_norm, double cell, int flags) {
  PlanFrame& f = ((Planner*)h)->frames[k];
  f.n = n; f.max_norm = max_norm; f.cell = cell; f.has_grid = flags & 1; f.has_tie = flags & 2; f.has_snor = flags & 4;
}

// the options of SearchOptions by their mvicp_set_option names; -> 0, or -1 for a name the policy does not read.  "tie_rule" forgets the
// history when the value changes, and "nn_cache" voids the cache, as mvicp_set_option does
int plan_set_option(void* h, const char* name, double v) {
  Planner* P = (Planner*)h;
  SearchOptions& o = P->opt;
  const std::string n(name);
  if (n == "list_reuse") o.list_reuse = v != 0.0;
  else if (n == "nn_cache") { o.nn_cache_enable = v != 0.0; P->hist.nn_cache_valid = false; }
  else if (n == "nn_tree_only") o.nn_tree_only = v != 0.0;
  else if (n == "nn_skip_far") o.nn_skip_far = v != 0.0;
  else if (n == "nn_cell") o.nn_cell = v != 0.0;
  else if (n == "tile_bounds") o.tile_bounds = (int)v;
  else if (n == "tile_cache") o.tile_cache = (int)v;
  else if (n == "tile_mfma") o.tile_mfma = (int)v;
  else if (n == "cache_mfma_ratio") o.cache_mfma_ratio = v;
  else if (n == "tile_mu") o.tile_mu = v;
  else if (n == "sel_bracket") o.sel_bracket = v != 0.0;
  else if (n == "sel_reuse") o.sel_reuse = v != 0.0;
  else if (n == "spec_eval") o.spec_enable = v != 0.0;
  else if (n == "spec2_eval") o.spec2_enable = v != 0.0;
  else if (n == "lin_pair") o.lin_pair = v != 0.0;
  else if (n == "auto_settle") o.auto_settle = v;
  else if (n == "auto_switch") o.auto_switch = v;
  else if (n == "tie_rule") { const bool on = v != 0.0; if (on != o.tie_rule) { o.tie_rule = on; P->hist.forget(P->E); } }
  else if (n == "tie_lazy") o.tie_lazy = v != 0.0;
  else return -1;
  return 0;
}

// plan_search at poses (n_frames x 16, column-major) / fixed (n_frames bytes or null).  -> the plan's status; *out = the plan
int plan_run(void* h, const double* poses, const unsigned char* fixed, float thresh, int nn_method, int exchange, int world, PlanOut* out) {
  Planner* P = (Planner*)h;
  P->poses.assign(poses, poses + 16 * (size_t)P->K);
  if (fixed) P->fixed.assign(fixed, fixed + P->K);
  SearchInputs& in = P->in;
  in.E = P->E; in.n_frames = P->K; in.esrc = P->esrc.data(); in.edst = P->edst.data(); in.owned = P->owned.data(); in.frames = P->frames.data();
  in.poses = P->poses.data(); in.fixed = fixed ? P->fixed.data() : nullptr; in.thresh = thresh; in.nn_method = nn_method;
  in.exchange = exchange != 0; in.world = world;
  SearchPlan& p = P->plan;
  p.active = P->active.data(); p.src_fixed = P->src_fixed.data(); p.xf = P->xf.data(); p.nsrc = P->nsrc.data(); p.dirty = P->dirty.data(); p.lohi = P->lohi.data();
  plan_search(in, P->opt, P->hist, p);
  *out = PlanOut{p.status, p.method, p.tile_lb, p.tile_cached, p.handed_over, p.cached_on_mfma, p.all_same, p.same_active_set, p.all_unchanged,
                 p.nothing_can_change, p.tie_skip, p.far_skip, p.far_narrow, p.tie_launched, p.far_launched, p.sel_skip,
                 p.use_bracket, p.spec_arm, p.spec2_plan, (int)p.tie_need.size(), p.eps_over_mu};
  return p.status;
}

// the per-edge rows of the last plan: ints = E x 6 (active, src_fixed, nsrc, same_edge, unchanged, dirty), reals = E x 3 (cache slot, lo, hi),
// tie_need = the frames that need a tree (n_tie_need of them)
void plan_rows(void* h, int* ints, double* reals, int* tie_need) {
  Planner* P = (Planner*)h;
  const SearchPlan& p = P->plan;
  for (int e = 0; e < P->E; ++e) {
    int* r = ints + 6 * e;
    r[0] = p.active[e]; r[1] = p.src_fixed[e]; r[2] = p.nsrc[e]; r[3] = p.same_edge[e]; r[4] = p.unchanged[e]; r[5] = p.dirty[e];
    reals[3 * e] = p.xf[(size_t)e * kEdgeXf + kXfCache]; reals[3 * e + 1] = p.lohi[2 * e]; reals[3 * e + 2] = p.lohi[2 * e + 1];
  }
  for (size_t k = 0; k < p.tie_need.size(); ++k) tie_need[k] = p.tie_need[k];
}

// the NN launch of the last plan is on the stream
void plan_queued(void* h) { Planner* P = (Planner*)h; record_queued(P->in, P->opt, P->plan, P->hist); }

// what arrived after the wait: res = (count, median d2) x E | armed, scales = E.  -> the queued first evaluation may be used
int plan_arrived(void* h, unsigned int tie_word, unsigned int far_word, const double* res, const double* scales, int redone) {
  Planner* P = (Planner*)h;
  return record_arrived(P->in, P->plan, P->hist, tie_word, far_word, res, scales, redone != 0) ? 1 : 0;
}

void plan_forget(void* h) { Planner* P = (Planner*)h; P->hist.forget(P->E); }                                   // reset, a failed search
void plan_explicit(void* h, int edge, int n, float weight) { ((Planner*)h)->hist.explicit_edge(edge, n, weight); }   // mvicp_set_correspondences
// mvicp_optimize ended: valid = a point / plane solve that returned OK
void plan_solved(void* h, int valid, int param, int plane, int robust) {
  SearchHistory& H = ((Planner*)h)->hist;
  H.spec_flags_valid = valid != 0;
  if (valid) { H.spec_param = param; H.spec_plane = plane; H.spec_robust = robust; } else H.last_cand_poses.clear();
}
// the last solve asked for an evaluation beyond its first, at `poses`
void plan_candidate(void* h, const double* poses, int plane, int robust) {
  Planner* P = (Planner*)h;
  P->hist.last_cand_poses.assign(poses, poses + 16 * (size_t)P->K); P->hist.last_cand_plane = plane; P->hist.last_cand_robust = robust;
}
// a few history fields the tests read back: auto_last_method, nn_cache_valid, sel_result_valid, sel_result_armed, corr_tie_seen, corr_far_seen
void plan_history(void* h, int* out) {
  const SearchHistory& H = ((Planner*)h)->hist;
  out[0] = H.auto_last_method; out[1] = H.nn_cache_valid; out[2] = H.sel_result_valid; out[3] = H.sel_result_armed; out[4] = (int)H.corr_tie_seen; out[5] = (int)H.corr_far_seen;
}

}  // extern "C"
