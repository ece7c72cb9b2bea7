// The search policy of mvicp_correspond, host-only: what a search is a function of (SearchInputs, SearchOptions), what earlier searches
// left behind (SearchHistory), and everything that is decided before the first HIP call (SearchPlan, plan_search).  Nothing here includes
// or calls HIP: the file compiles with a plain host compiler (-std=c++17 -ffp-contract=off) and tests/plan_harness.cpp drives it without a
// GPU.  The executor that uploads, launches, exchanges and waits is csrc/api.cpp (correspond_once).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mvicp.h"

namespace mvicp {

constexpr int kEdgeXf = 40;          // doubles per edge of the query-transform block, laid out as:
constexpr int kXfRigid = 24;         //   [0, 24): Rs(9) ts(3) Rdinv(9) td(3), column-major (what xf_point reads, nn_metric.h)
constexpr int kXfCache = 24;         //   temporal-cache switch (>= 0: on, value = rounding allowance in metres; < 0: off)
constexpr int kXfDM = 25;            //   dM (9, column-major) and
constexpr int kXfDv = 34;            //   dv (3): change of the query map q = M p + v since the last search, so a query moved by exactly |dM p + dv|
constexpr int kXfPad = 37;           //   [37, kEdgeXf): zero padding

// smallest double x such that the correctly rounded sqrt(x) >= t  ==>  (sqrt(d2) < t)  <=>  (d2 < x)
inline double sqrt_bound(double t) {
  double x = t * t;
  while (std::sqrt(x) >= t && x > 0.0) x = std::nextafter(x, 0.0);
  while (std::sqrt(x) < t) x = std::nextafter(x, INFINITY);
  return x;
}

// Eigen 3x3 inverse (cofactor form), column-major — frame.cpp:118 `dstCloud.pose.linear().inverse()`.
inline void inverse3(const double* m, double* r) {
#define M(i, j) m[(i) + 3 * (j)]
#define COF(i, j) (M(((i) + 1) % 3, ((j) + 1) % 3) * M(((i) + 2) % 3, ((j) + 2) % 3) - M(((i) + 1) % 3, ((j) + 2) % 3) * M(((i) + 2) % 3, ((j) + 1) % 3))
  const double c00 = COF(0, 0), c10 = COF(1, 0), c20 = COF(2, 0);
  const double det = (c00 * M(0, 0) + c10 * M(1, 0)) + c20 * M(2, 0);
  const double invdet = 1.0 / det;
  r[0] = c00 * invdet; r[3] = c10 * invdet; r[6] = c20 * invdet;
  r[1] = COF(0, 1) * invdet; r[4] = COF(1, 1) * invdet; r[7] = COF(2, 1) * invdet;
  r[2] = COF(0, 2) * invdet; r[5] = COF(1, 2) * invdet; r[8] = COF(2, 2) * invdet;
#undef COF
#undef M
}

// The query transform of a directed pair src -> dst (frame.cpp:117-118,131,136), the first 24 doubles of an edge's kEdgeXf:
// Rs(9) ts(3) Rd^-1(9) td(3), column-major.  mvicp_correspond and mvicp_overlap both build theirs here.
inline void fill_query_xf(const double* Ps, const double* Pd, double* x) {
  double Rd[9];
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) { x[i + 3 * j] = Ps[i + 4 * j]; Rd[i + 3 * j] = Pd[i + 4 * j]; }
  for (int i = 0; i < 3; ++i) { x[9 + i] = Ps[12 + i]; x[21 + i] = Pd[12 + i]; }
  inverse3(Rd, x + 12);
}

// The affine form of a query transform block x (fill_query_xf): q = M p + v with M = Rd^-1 Rs (9, column-major), v = Rd^-1 (ts - td) (3).
// The kernels never evaluate it (they run xf_point); its change between two searches is the displacement cache_eps reads.
inline void query_affine(const double* x, double* Mq) {
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) Mq[i + 3 * j] = x[12 + i] * x[0 + 3 * j] + x[12 + i + 3] * x[1 + 3 * j] + x[12 + i + 6] * x[2 + 3 * j];
  const double dt[3] = {x[9] - x[21], x[10] - x[22], x[11] - x[23]};
  for (int i = 0; i < 3; ++i) Mq[9 + i] = x[12 + i] * dt[0] + x[12 + i + 3] * dt[1] + x[12 + i + 6] * dt[2];
}

// The rounding allowance of the temporal cache (nn_cache.h: cache_eps adds it to |dM p + dv|): a bound on everything that separates the
// displacement the kernel computes from the distance between the two ROUNDED queries the kernels really searched with — the roundings of
// xf_point (nn_metric.h), of query_affine, and of the kernel's fl(dM p + dv).  With u = 2^-53, |p| <= r, Frobenius norms, to first order and
// for both searches, each with its own block x = (R, ts, Ri, td):
//     |q^_new - q^_old| <= |e^| (1 + 1e-9) + u sum over both blocks of ||Ri|| (|ts| + 16 ||R|| r + 13 |ts - td|)
// (derivation: DESIGN.md section 3.4; the leading term lives at the size of ts, NOT of v = Ri (ts - td): georeferenced scans).  The allowance
// is that sum with 2 u = 2^-52: the spare factor covers the second-order terms and the roundings of the norms, of r and of this sum.  Blocks
// that are bit-identical give the same queries bit for bit: 0, which the kernels read as "nothing moved"; any other pair gives a positive value.
inline double cache_allowance_xf(const double* x_old, const double* x_new, double r) {
  if (std::memcmp(x_old, x_new, sizeof(double) * kXfRigid) == 0) return 0.0;
  double b = 0.0;
  for (const double* x : {x_old, x_new}) {
    double fr = 0.0, fi = 0.0;
    for (int k = 0; k < 9; ++k) { fr += x[k] * x[k]; fi += x[12 + k] * x[12 + k]; }
    const double dt[3] = {x[9] - x[21], x[10] - x[22], x[11] - x[23]};
    const double ts = std::sqrt(x[9] * x[9] + x[10] * x[10] + x[11] * x[11]), dtn = std::sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]);
    b += std::sqrt(fi) * (ts + 16.0 * std::sqrt(fr) * r + 13.0 * dtn);
  }
  return std::max(0x1p-52 * b, std::numeric_limits<double>::min());
}

// The options the policy reads (mvicp_set_option writes here; the launchers that need one read it here): one copy, no per-call snapshot.
struct SearchOptions {
  bool list_reuse = true;          // skip compaction + gather for edges whose list did not change
  bool nn_cache_enable = true;     // option "nn_cache": the temporal cache
  bool nn_tree_only = false;
  bool nn_skip_far = false;        // PROFILING ONLY: leave unresolved queries unresolved (wrong results)
  bool nn_cell = false;            // grid method: wave-cooperative cell-staging kernel (nn_cell_kernel) instead of the per-lane hash kernel.  Exact and
                                   // tested at full size, but measured SLOWER on MI355X (cfg4 rounds 3-7: 5.4 / 3.2 / 2.3 / 1.7 / 1.0 ms vs 2.3 / 1.8 / 2.6 / 0.9 / 0.6 ms,
                                   // profiles/r02_nn_cell_experiment.txt): off by default
  int tile_bounds = 1;             // 1: the AUTO round that would hand over to the grid kernel runs the tile kernel's BND build instead (it leaves the
                                   // temporal-cache bounds, so the grid kernel starts with cache hits one round later and the uncached grid round — the
                                   // slowest of a registration — never runs); 2: every tile round leaves bounds (tests); 0: off
  int tile_cache = 1;              // AUTO, after the hand-over: rounds whose transforms still move run the tile kernel's bounds-leaving build WITH the
                                   // temporal-cache check as its prologue (missed lanes are searched wave-cooperatively) instead of the grid kernel
  int tile_mfma = 1;               // tile method: 1 = the screen of an opened tile runs on the matrix pipe (nn_mfma.hip) except in cache-aware rounds, 2 = always,
                                   // 0 = never (the fp32 VALU screen of nn_tile.hip)
  double cache_mfma_ratio = 3.0;   // cache-aware rounds run on the matrix-pipe build when the median displacement bound of the queries exceeds this many guard bands
                                   // (eps / mu; 0 = never: always nn_tile_kernel).  Measured (profiles/r06_tile_ab.txt): eps / mu <= 2.2 <-> hit rates >= 0.86 (nn_tile_kernel +
                                   // miss_block faster), eps / mu >= 3.4 <-> hit rates <= 0.77 (nn_mfma_kernel 6-12 % faster)
  double tile_mu = 0.02;           // BND guard band as a fraction of the target's hash-cell edge (same role as prune_rho in the grid kernel); round 3 sweep on cfg4
                                   // (hand-over round + the two cache-aware rounds after it): 0.02 -> 2.06 ms, 0.05 -> 2.11, 0.1 -> 2.23, 0.2 -> 2.45
  bool sel_bracket = true;         // use the one-pass bracket select once the medians have settled
  bool sel_reuse = true;           // no select launch in a single-rank search in which no list can change (0: launch it every search)
  bool spec_enable = true;         // option "spec_eval": queue the first evaluation of the next solve behind the select (api.cpp)
  bool spec2_enable = true;        // ... and at a fixed point the last solve's candidate evaluation behind it
  bool lin_pair = true;            // two queued evaluations of a fixed-point round go as ONE paired launch (0: two launches, a copy between them)
  double auto_settle = 0.5;        // AUTO: "settled" = the median distance is above this fraction of the one before
  double auto_switch = 1.0;        // AUTO (nn_cell): hand over from the tile kernel to the grid method once the median distance is below this many hash cells
  bool tie_rule = true;            // exact distance ties are decided as nanoflann decides them (first visited; nn_tie.hip); false: lowest original index
  bool tie_lazy = true;            // single rank: the reference-equivalent trees (kdvisit.h) are built when a search first REPORTS a tie on a target without one (the
                                   // search is then repeated once), like the reference's own lazily built index (frame.cpp:188-193) — synthetic clouds never tie, and
                                   // the eager build was most of cfg5's set-up time.  N > 1 ranks build them at mvicp_set_graph (a repeated search is a collective)
};

// mvicp_correspond — cross-round state at a glance.  A search is a PURE FUNCTION of (clouds, graph, poses, fixed mask, cutoff): every field below
// only decides HOW FAST the same answer is found, and tests/test_gpu_parity.py::test_correspond_regime_transitions_match_a_fresh_context checks
// after every round of randomly perturbed registrations that the answer equals a fresh context's.  mvicp_reset_history, a search that does not
// return OK (mvicp_correspond's Forget guard: every error return, an exception, a poisoned exchange) and a change of the "tie_rule" option
// (forget) drop all of it — "reset" in the last column stands for all three (tests/test_gpu_search_state.py).
//   field                         written by                               read by / meaning                                    invalidated by
//   nn_cache_valid, _thresh       record_queued (grid / BND tile round)    temporal cache may be consulted next search          cutoff change, set_correspondences, options, reset
//   nn_cache_edge[e]              record_queued (= active mask)            edge e was searched last time: seeds + bounds usable   fixed-mask change (per edge), reset
//   prev_q / prev_xf[e]           plan_search's per-edge loop              dM, dv of the temporal cache; bit-identical transform  every search rewrites them; a search that does not return OK, reset
//   list_valid[e], explicit_list  record_queued / set_correspondences      the edge's compacted list may be maintained in place  set_correspondences, recompute_normals (dst), reset
//   sel_med1/2[e]                 record_arrived                           one-pass bracket select once the median has settled   inactive edge, set_correspondences, reset
//   sel_result_valid, _armed      record_arrived (single rank)             no select launch in a search in which no list can change   any search that does not return OK, set_graph, set_correspondences, reset
//   auto_prev_dist, auto_last_method   plan_search / record_queued         hand-over tile -> grid, "already handed over"          set_graph, reset
//   corr_tie_seen, corr_far_seen  record_arrived (own launches only)       tie fix-up / far launch may be skipped at a fixed point  any search that is not bit-identical; reset
//   prev_grid_kernel              record_queued                            corr_far_seen describes the last search                every search rewrites it
//   spec_flags_valid, spec_param/plane/robust   mvicp_optimize             arm the queued first evaluation of the NEXT solve      failed solve / search, reset
//   last_cand_poses, _plane, _robust   an evaluation beyond a solve's first   the second queued evaluation predicts it again      set_graph, failed solve, reset
//   last_rms                      mvicp_optimize                           nn_cell policy only                                    consumed by record_queued
//   qpos_valid[e]                 record_queued                            d_qpos / second / cd2 = the last search's result (export)  set_correspondences, failed search, reset
//   have_corr, h_count, h_weight  record_arrived / set_correspondences     the results; AUTO's median distance                   set_graph, reset
// What stays on the context because it is not a function of the searches alone (api.cpp forget_history adds it to forget):
//   spec_ready, spec_poses        end of a search                          evaluate_blocks may serve the first evaluation from it  consumed by the next evaluation, any list change
//   export_valid                  ensure_export                            h_export holds the lists as they are on the device     every search that can change a list, set_correspondences, reset
//   corr_epoch[e]                 end of a search                          callers skip copying a list whose epoch they hold      bumped unless the edge's inputs are bit-identical to last search's
struct SearchHistory {
  bool have_corr = false;
  bool nn_cache_valid = false; float nn_cache_thresh = -1.f;
  std::vector<char> nn_cache_edge;  // edges searched (active) in the last search
  std::vector<double> prev_q;       // E x 12: query map M = Rd^-1 Rs (9, col-major) and v = Rd^-1 (ts - td) of the last search
  std::vector<double> prev_xf;      // E x 24: the raw query transform (Rs ts Rd^-1 td) of the last search: bit-identical -> queries bit-identical
  std::vector<char> list_valid;     // E: d_qpos / lists describe last round's result of this edge
  std::vector<char> explicit_list;  // E: the edge's list was installed by mvicp_set_correspondences (arbitrary order / repeats: no d_qpos for it)
  std::vector<char> qpos_valid;     // E: d_qpos / d_second / d_cd2 describe the LAST SEARCH's result of this edge (what the export reads).  Unlike list_valid
                                    // (= the list may be maintained in place next round) it survives mvicp_recompute_normals, which only re-gathers operands
  std::vector<double> sel_med1, sel_med2;   // per searched edge (single rank: owned; with an exchange: every rank's): median d2 of the last / the one-before-last round (< 0: unknown)
  bool sel_result_valid = false;    // the last search on this context finished its select: d_median, d_a and the mapped (count, median d2) pairs are that select's
  bool sel_result_armed = false;    // ... and that select also wrote the SoftLOne scales (d_a and their mapped copy)
  double auto_prev_dist = 0.0; int auto_last_method = -1;   // MVICP_NN_AUTO policy state
  double last_rms = -1.0;           // RMS residual at the end of the last mvicp_optimize since the last search (< 0: none): predicts the next NN distances
  unsigned int corr_tie_seen = 1u, corr_far_seen = 1u;   // what the LAST search's own fix-up / far launch reported (read after its wait; 1 = unknown).
                                    // mvicp_nn_query runs the same launches and overwrites the mapped words, so the skip decisions use these copies
  bool prev_grid_kernel = false;    // the previous search ran nn_grid_kernel + nn_far_kernel (so corr_far_seen describes it)
  bool spec_flags_valid = false; int spec_param = 0, spec_plane = 0, spec_robust = 0;   // the last solve's parameterization / cost flags
  std::vector<double> last_cand_poses;   // poses of the last evaluation a solve asked for beyond its first (the prediction for the next solve's candidate)
  int last_cand_plane = -1, last_cand_robust = -1;
  std::vector<int> h_count;         // E, valid after correspond / set_correspondences (owned edges)
  std::vector<float> h_weight;      // E

  // everything earlier searches left behind is dropped: the next search is a first search
  void forget(int E) {
    nn_cache_valid = false; nn_cache_thresh = -1.f;
    prev_q.assign((size_t)E * 12, 0.0); prev_xf.assign((size_t)E * kXfRigid, 0.0);
    nn_cache_edge.assign(E, 0);                      // no seeds, no temporal cache: d_nn_idx / d_nn_lb are dead until the next search rewrites them
    auto_prev_dist = 0.0; auto_last_method = -1; last_rms = -1.0; prev_grid_kernel = false;
    corr_tie_seen = corr_far_seen = 1u;
    list_valid.assign(E, 0);                         // every list is re-compacted and re-gathered
    qpos_valid.assign(E, 0);
    sel_med1.assign(E, -1.0); sel_med2.assign(E, -1.0);
    sel_result_valid = false;
    spec_flags_valid = false;
    last_cand_poses.clear();
    have_corr = false;
    std::fill(h_count.begin(), h_count.end(), 0); std::fill(h_weight.begin(), h_weight.end(), 0.f);
  }
  // mvicp_set_graph: every per-edge row gets the new graph's size and describes no search; what the last solve left (spec_*, last_rms) stays
  void new_graph(int E) {
    h_count.assign(E, 0); h_weight.assign(E, 0.f); have_corr = false;
    sel_med1.assign(E, -1.0); sel_med2.assign(E, -1.0);
    nn_cache_valid = false; prev_q.assign((size_t)E * 12, 0.0); prev_xf.assign((size_t)E * kXfRigid, 0.0); nn_cache_edge.assign(E, 0);
    auto_prev_dist = 0.0; auto_last_method = -1; corr_tie_seen = corr_far_seen = 1u;
    list_valid.assign(E, 0); explicit_list.assign(E, 0); qpos_valid.assign(E, 0);
    sel_result_valid = false; sel_result_armed = false;
    last_cand_poses.clear();
  }
  // mvicp_set_correspondences: the edge's list is the caller's from now on
  void explicit_edge(int edge, int n, float weight) {
    nn_cache_valid = false;
    list_valid[edge] = 0; explicit_list[edge] = 1; qpos_valid[edge] = 0;
    sel_med1[edge] = sel_med2[edge] = -1.0;
    sel_result_valid = false;   // d_count, d_cd2 and d_a of this edge are no longer the last select's
    h_count[edge] = n; h_weight[edge] = weight;
    have_corr = true;
  }
};

// What a search is a function of, without device pointers.  The arrays are the caller's and outlive the call.
struct PlanFrame { int n = 0; double max_norm = 0.0, cell = 0.0; bool has_grid = false, has_tie = false, has_snor = false; };   // cell: the hash cell edge; has_snor: sorted normals exist
struct SearchInputs {
  int E = 0, n_frames = 0;
  const int* esrc = nullptr; const int* edst = nullptr; const char* owned = nullptr;   // the graph (E each)
  const PlanFrame* frames = nullptr;                                                    // n_frames
  const double* poses = nullptr; const unsigned char* fixed = nullptr;                  // n_frames x 16 column-major; null = no frame fixed
  float thresh = 0.f; int nn_method = MVICP_NN_AUTO;
  bool exchange = false; int world = 1;                                                 // an exchange is configured (RCCL or host-staged) / its size
};

// Everything decided before the first HIP call.  The per-edge rows the device or the launchers read go straight into memory the caller
// provides (the pinned mirror of the control block; the context's active / src_fixed masks); the rest is storage of the plan object, which
// the context keeps so that a search allocates nothing once the graph is set.
struct SearchPlan {
  // caller-provided: set before plan_search
  char* active = nullptr;          // E: owned && src not fixed
  char* src_fixed = nullptr;       // E: the edge's source frame is fixed
  double* xf = nullptr;            // E x kEdgeXf
  int* nsrc = nullptr;             // E: N_src if active else 0
  int* dirty = nullptr;            // E: != 0 -> the edge's list is re-compacted and re-gathered whatever the kernels report
  double* lohi = nullptr;          // E x 2: bracket of the one-pass select (0, 0 without one)
  // per edge
  std::vector<char> same_edge;     // the edge's query transform is bit-identical to last search's (and the temporal cache is on for it)
  std::vector<char> unchanged;     // the edge's list after this search IS last search's, bit for bit: it keeps its epoch
  std::vector<double> eps_ratio;   // per active edge: displacement bound of its queries since the last search / guard band mu
  std::vector<int> tie_need;       // frames that need a tie tree before the search
  // over the graph
  bool all_same = true, same_active_set = false, all_unchanged = true;
  // kernel choice
  int method = MVICP_NN_TILE;
  bool tile_lb = false, tile_cached = false, handed_over = false;
  double eps_over_mu = -1.0;       // median of eps_ratio when the two tile builds were weighed (< 0: not weighed)
  bool cached_on_mfma = false;
  // skip decisions
  bool nothing_can_change = false, tie_skip = false, far_skip = false, far_narrow = false, tie_launched = false, far_launched = false, sel_skip = false;
  // select and queued evaluations
  bool use_bracket = false, spec_arm = false, spec2_plan = false;
  int status = MVICP_OK;           // MVICP_ERR_ARG: unknown nn_method
};

// plan_search, first part: the per-edge rows — masks, transform block with the temporal cache's dM, dv and allowance, same_edge, unchanged —
// and the frames that need a tie tree.  Rewrites prev_xf / prev_q.
inline void plan_edges(const SearchInputs& in, const SearchOptions& opt, SearchHistory& h, SearchPlan& p) {
  const int E = in.E;
  const float thresh = in.thresh;
  const unsigned char* fixed = in.fixed;
  // per-edge query transforms (frame.cpp:117-118,131,136) + active mask (frame.cpp:93)
  p.same_edge.assign(E, 0);
  // the edge's list after this search IS last search's, bit for bit: a search is a pure function of (clouds, transform, cutoff), and all three are
  // last search's — whichever kernel runs.  Such an edge keeps its epoch (mvicp_correspondence_epochs), and if every edge does, the export too.
  p.unchanged.assign(E, 0);
  p.eps_ratio.clear();
  const bool hist_ok = h.have_corr && (int)h.nn_cache_edge.size() == E && h.nn_cache_thresh == thresh && (int)h.qpos_valid.size() == E;
  p.same_active_set = (int)h.nn_cache_edge.size() == E;   // the set of searched edges is last search's (a changed `fixed` mask changes it)
  for (int e = 0; e < E; ++e) {
    const PlanFrame& fs = in.frames[in.esrc[e]];
    const PlanFrame& fd = in.frames[in.edst[e]];
    p.active[e] = in.owned[e] && !(fixed && fixed[in.esrc[e]]);
    p.src_fixed[e] = fixed && fixed[in.esrc[e]];
    if (p.same_active_set && (p.active[e] != 0) != (h.nn_cache_edge[e] != 0)) p.same_active_set = false;
    p.nsrc[e] = p.active[e] ? fs.n : 0;
    double* x = p.xf + (size_t)e * kEdgeXf;
    fill_query_xf(in.poses + 16 * (size_t)in.esrc[e], in.poses + 16 * (size_t)in.edst[e], x);
    // temporal cache: q = M p + v with M = Rd^-1 Rs, v = Rd^-1 (ts - td).  Between two searches every query of the edge
    // moves by at most ||dM||_F max|p| + |dv|  (+ the rounding allowance of cache_allowance_xf).
    double Mq[12];
    query_affine(x, Mq);
    double* pq = &h.prev_q[(size_t)e * 12];
    for (int k = 0; k < 12; ++k) x[kXfDM + k] = Mq[k] - pq[k];
    const double rmax = fs.max_norm;
    if (p.active[e]) {
      // how far this edge's queries can have moved since the last search, in units of the bounds-leaving builds' guard band: what decides the
      // temporal-cache hit rate of a cache-aware round before it runs (a hit needs d_new < d_old + mu - eps)
      double fro = 0.0;
      for (int k = 0; k < 9; ++k) fro += x[kXfDM + k] * x[kXfDM + k];
      const double eps_e = std::sqrt(fro) * rmax + std::sqrt(x[kXfDv] * x[kXfDv] + x[kXfDv + 1] * x[kXfDv + 1] + x[kXfDv + 2] * x[kXfDv + 2]);
      const double mu_e = opt.tile_mu * fd.cell;
      p.eps_ratio.push_back(mu_e > 0.0 ? eps_e / mu_e : 1e300);
    }
    const bool cache_on = h.nn_cache_valid && opt.nn_cache_enable && p.active[e] && (int)h.nn_cache_edge.size() == E && h.nn_cache_edge[e] &&
                          h.nn_cache_thresh == thresh;
    // allowance for the rounding of the fp64 query map itself (both evaluations) and of dM, dv: cache_allowance_xf.
    // A transform that is BIT-IDENTICAL to last search's (a converged registration: the LM ends without stepping) reproduces every
    // query bit for bit: no allowance, and dM = dv = 0 below, so the kernel sees eps == 0 and re-verifies without rewriting anything.
    double* pxf = &h.prev_xf[(size_t)e * kXfRigid];
    const bool same_xf = std::memcmp(pxf, x, sizeof(double) * kXfRigid) == 0;
    if (!in.owned[e]) p.unchanged[e] = 1;   // (another rank's edge: nothing of it lives here)
    else if (p.active[e]) p.unchanged[e] = hist_ok && h.nn_cache_edge[e] && h.qpos_valid[e] && !h.explicit_list[e] && same_xf;
    else p.unchanged[e] = hist_ok && !h.nn_cache_edge[e] && !h.explicit_list[e] && h.h_count[e] == 0;   // not searched now, not searched then: stays empty
    x[kXfCache] = cache_on ? cache_allowance_xf(pxf, x, rmax) : -1.0;
    p.same_edge[e] = cache_on && same_xf;
    std::memcpy(pxf, x, sizeof(double) * kXfRigid);
    for (int k = kXfPad; k < kEdgeXf; ++k) x[k] = 0.0;
    std::memcpy(pq, Mq, sizeof(Mq));
  }
  // a cloud uploaded after mvicp_set_graph has no tie tree yet (the reference builds its index lazily as well, frame.cpp:188-193); a single
  // rank with tie_lazy builds them only when a search reports a tie (mvicp_correspond)
  p.tie_need.clear();
  if (opt.tie_rule && !(opt.tie_lazy && in.world == 1))
    for (int e = 0; e < E; ++e) if (p.active[e] && !in.frames[in.edst[e]].has_tie) p.tie_need.push_back(in.edst[e]);
  p.all_same = true;   // every active edge's query transform is bit-identical to last search's
  for (int e = 0; e < E; ++e) if (p.active[e] && !p.same_edge[e]) p.all_same = false;
}

// plan_search, second part: which kernel — the AUTO policy, the hand-over, cache-aware tile rounds and their build.  Writes auto_prev_dist.
inline void choose_kernel(const SearchInputs& in, const SearchOptions& opt, SearchHistory& h, SearchPlan& p) {
  const int E = in.E;
  int method = in.nn_method;
  if (method == MVICP_NN_AUTO) {
    // Two exact kernels, two regimes.  While the poses still move by more than the spacing of the points, nearly every
    // query needs a fresh search and the wave-cooperative tile kernel (seeded with last round's neighbours) is fastest.
    // Once the registration settles, the hash-grid kernel wins: its temporal cache answers a query whose neighbour provably
    // did not change with one distance evaluation.  The switch costs one uncached grid round, so it is made when the
    // median correspondence distance has stopped contracting (last > half of the one before) — or, with a single round
    // of history, when it is already well inside a hash cell.
    method = MVICP_NN_TILE;
    if (h.have_corr) {
      double dist = 0.0, cell = 0.0;
      int m = 0;
      for (int e = 0; e < E; ++e)
        if (h.h_count[e] > 0) { dist += h.h_weight[e] / 1.5; cell += in.frames[in.edst[e]].cell; ++m; }
      if (m > 0) {
        dist /= m; cell /= m;
        const bool settled = h.auto_prev_dist > 0.0 ? dist > opt.auto_settle * h.auto_prev_dist : dist < 0.5 * cell;
        if (opt.nn_cell) {
          // cell-staging grid kernel: it resolves a query whose neighbour is within about a cell of it (home block + ball) at a cost
          // that follows that distance, not the cache hit rate — so it takes over as soon as the queries are EXPECTED to land that
          // close: the smaller of last round's median distance and the residual the LM solve has just left (RMS over all
          // correspondences, with a floor of a fraction of a cell for the sampling of the surface)
          double pred = dist;
          if (h.last_rms >= 0.0) pred = std::min(pred, std::sqrt(h.last_rms * h.last_rms + 0.09 * cell * cell));
          if (pred < opt.auto_switch * cell || h.auto_last_method == MVICP_NN_GRID) method = MVICP_NN_GRID;
        } else if (dist < 1.5 * cell && (settled || h.auto_last_method == MVICP_NN_GRID)) method = MVICP_NN_GRID;
        h.auto_prev_dist = dist;
      }
    }
  }
  if (method == MVICP_NN_GRID || method == MVICP_NN_TILE) {
    for (int e = 0; e < E; ++e)
      if (p.active[e] && (!in.frames[in.edst[e]].has_grid || !in.frames[in.esrc[e]].has_grid)) method = MVICP_NN_BRUTE;
  }
  // The round in which AUTO hands over to the grid kernel would be an UNCACHED grid round (every query searched through the hash:
  // 2.4-2.6 ms on cfg4, the slowest round after the first).  Instead the tile kernel runs once more in its BND build (~1.2 ms), which
  // also leaves the per-query lower bounds the temporal cache needs; the grid kernel takes over one round later, with cache hits.
  const bool is_auto = in.nn_method == MVICP_NN_AUTO;
  p.tile_lb = false; p.handed_over = false;
  if (is_auto && method == MVICP_NN_GRID && h.auto_last_method == MVICP_NN_TILE && opt.tile_bounds >= 1 &&
      opt.nn_cache_enable && !opt.nn_cell) { method = MVICP_NN_TILE; p.tile_lb = true; p.handed_over = true; }
  if (method == MVICP_NN_TILE && opt.tile_bounds >= 2 && opt.nn_cache_enable) p.tile_lb = true;
  // Cache-aware tile rounds (round 3).  After the hand-over the grid kernel answers cache hits at streaming speed but pays 1.5-2 ns for
  // every isolated miss (per-lane hash probing), which dominates the rounds in which the poses still move a little (hit rates 74-99 %).
  // Those rounds run the tile kernel's bounds-leaving build with the cache check as its prologue instead: a missed lane is searched by
  // its wave, cooperatively.  Once every transform is bit-identical to last search's (the fixed point) the grid kernel's verify pass is
  // the cheaper one and takes over.
  p.tile_cached = false;
  if (is_auto && method == MVICP_NN_GRID && !p.handed_over && opt.tile_cache && opt.tile_bounds >= 1 && h.nn_cache_valid &&
      opt.nn_cache_enable && !opt.nn_cell && !p.all_same) { method = MVICP_NN_TILE; p.tile_lb = true; p.tile_cached = true; p.handed_over = true; }
  // experiment (round 6, "tile_cache" = 2): the cache prologue in EVERY tile round that follows a bounds-leaving one (with "tile_bounds" = 2: from
  // round 3 on), not only after the hand-over — measures how early the temporal cache starts to hit (profiles/r06_tile_ab.txt)
  if (method == MVICP_NN_TILE && !p.tile_cached && opt.tile_cache >= 2 && p.tile_lb && h.nn_cache_valid && opt.nn_cache_enable && !p.all_same) p.tile_cached = true;
  p.method = method;
  // Cache-aware rounds: which build?  With most lanes finished by the cache, nn_tile_kernel (per-lane box tests, miss_block) wins; with hit rates
  // below ~80 % the matrix-pipe build does (cfg4_partial rounds 5-13: -4 ... -10 %, profiles/r06_tile_ab.txt).  The hit rate is not known before
  // the launch, but what decides it is: the median displacement bound of the queries in units of the guard band (eps / mu).
  p.cached_on_mfma = false; p.eps_over_mu = -1.0;
  if (method == MVICP_NN_TILE && p.tile_cached && opt.tile_mfma == 1 && opt.cache_mfma_ratio > 0.0 && !p.eps_ratio.empty()) {
    std::nth_element(p.eps_ratio.begin(), p.eps_ratio.begin() + p.eps_ratio.size() / 2, p.eps_ratio.end());
    p.eps_over_mu = p.eps_ratio[p.eps_ratio.size() / 2];
    p.cached_on_mfma = p.eps_over_mu > opt.cache_mfma_ratio;
  }
}

// 1. The plan of one search.  Writes prev_xf, prev_q, auto_prev_dist and (for the edges about to be searched) qpos_valid of the history, as
// the search always did: a search that does not return OK forgets the history anyway (mvicp_correspond's Forget guard).
inline void plan_search(const SearchInputs& in, const SearchOptions& opt, SearchHistory& h, SearchPlan& p) {
  const int E = in.E;
  plan_edges(in, opt, h, p);
  choose_kernel(in, opt, h, p);
  const int method = p.method;
  const bool is_auto = in.nn_method == MVICP_NN_AUTO;
  // an edge may keep last round's compacted list only if a kernel that checks every query's acceptance and patches changed
  // neighbours in place runs (the grid kernel, the tile kernel: nn_list.h) and the list on the device really is last round's result
  // for this edge
  const bool grid_lists = method == MVICP_NN_GRID && !opt.nn_tree_only && !opt.nn_skip_far;
  const bool keep_lists = (method == MVICP_NN_TILE || grid_lists) && opt.list_reuse;
  for (int e = 0; e < E; ++e) p.dirty[e] = (keep_lists && p.active[e] && h.list_valid[e]) ? 0 : 1;
  // One-pass bracket select (corr.hip) instead of the two-pass anchored select: only when EVERY searched edge has a median that has
  // settled (last two rounds within 0.1 %); the bracket is +-0.6 % in d2 around the last one.  With N > 1 ranks the medians of ALL edges
  // arrive in the exchanged buffer (record_arrived keeps them), and every searched edge of the graph is asked, not only this rank's: the
  // ranks then take the decision a single process takes.  A rank that asked its own edges alone armed a bracket whenever the unsettled
  // edges happened to be a peer's; the next medians left it, every rank ran the select again (redo_select: a second launch and a second
  // exchange) and the queued evaluation was dropped on all of them, where a single process does neither.
  p.use_bracket = opt.sel_bracket && h.have_corr;
  for (int e = 0; e < E; ++e) {
    p.lohi[2 * e] = p.lohi[2 * e + 1] = 0.0;
    if (!(in.exchange ? !p.src_fixed[e] : (bool)p.active[e])) continue;
    const double m1 = h.sel_med1[e], m2 = h.sel_med2[e];
    if (!(m1 > 0.0 && m2 > 0.0 && std::fabs(m1 - m2) <= 0.001 * m1)) { p.use_bracket = false; continue; }
    if (p.active[e]) { p.lohi[2 * e] = m1 * 0.994; p.lohi[2 * e + 1] = m1 * 1.006; }
  }
  // A search whose every edge has last round's exact transform and a valid list reproduces every query bit for bit: no list can
  // change, so the (data-dependent, early-exiting) list-maintenance kernels — dirty-flag reduction, compaction, gather — are not
  // even launched.
  // (not with the cell-staging variant: nn_cell_kernel has no bit-identical-query shortcut, so a fixed-point round is not a pure no-op there)
  p.nothing_can_change = grid_lists && opt.list_reuse && p.same_active_set && !opt.nn_cell;
  for (int e = 0; e < E && p.nothing_can_change; ++e)
    if (p.active[e] && !(p.same_edge[e] && p.dirty[e] == 0)) p.nothing_can_change = false;
  // ... and the tie fix-up (nn_tie.hip) neither, if last round's search reported no tie: the same queries meet the same targets
  p.tie_skip = p.nothing_can_change && h.corr_tie_seen == 0u;
  // ... nor the far launch after a grid round without far queries
  p.far_skip = p.nothing_can_change && h.corr_far_seen == 0u && h.prev_grid_kernel && method == MVICP_NN_GRID;
  p.tie_launched = opt.tie_rule && !p.tie_skip; p.far_launched = method == MVICP_NN_GRID && !p.far_skip;
  p.far_narrow = is_auto && method == MVICP_NN_GRID && h.nn_cache_valid && opt.nn_cache_enable && p.all_same;   // the fixed point: (almost) every query is a cache hit
  // Speculative first evaluation of the solve that follows (see common.h).  Every rank decides for itself (its own last solve set
  // the flags); with N > 1 ranks the decisions are SUMMED in the "armed" slot of the one exchanged buffer and the queued blocks are
  // used only if every rank armed — a rank that did not arm still takes part in the same collective with the same size.
  p.spec_arm = opt.spec_enable && h.spec_flags_valid;
  if (p.spec_arm && h.spec_plane)
    for (int e = 0; e < E; ++e) if (!p.src_fixed[e] && in.frames[in.edst[e]].n > 0 && !in.frames[in.edst[e]].has_snor) p.spec_arm = false;
  // second queued evaluation: this search's poses are last search's bit for bit, so the solve that follows will ask for last solve's candidate again
  p.spec2_plan = p.spec_arm && !in.exchange && opt.spec2_enable && p.all_same && p.same_active_set && h.have_corr &&
                 h.last_cand_poses.size() == 16 * (size_t)in.n_frames && h.last_cand_plane == h.spec_plane && h.last_cand_robust == h.spec_robust;
  // ... and the median select neither (single rank): the median of an edge is a function of its d2 list and its count, nothing rewrites either in such
  // a search, and the last search's select finished — d_median, d_a (the select's own values, or the host's bit-identical mirror uploaded by an
  // evaluation since) and the mapped (count, median d2) pairs ARE this search's result.  Only the "armed" slot is this search's own: the host writes
  // it.  With N > 1 ranks that tail lives in the exchanged buffer and is summed in place, so it is rewritten every search.
  p.sel_skip = !in.exchange && opt.sel_reuse && p.nothing_can_change && h.sel_result_valid && (!p.spec_arm || h.sel_result_armed);
  p.status = (method != MVICP_NN_BRUTE && method != MVICP_NN_GRID && method != MVICP_NN_TILE) ? MVICP_ERR_ARG : MVICP_OK;   // (an argument error: the same on every rank)
  p.all_unchanged = true;
  for (int e = 0; e < E; ++e) { if (!p.unchanged[e]) p.all_unchanged = false; if (p.status == MVICP_OK && p.active[e]) h.qpos_valid[e] = 0; }   // (set again once the NN stage is queued)
}

// 2. What a queued search leaves behind: called once the NN launch of the plan is on the stream.
inline void record_queued(const SearchInputs& in, const SearchOptions& opt, const SearchPlan& p, SearchHistory& h) {
  h.prev_grid_kernel = p.method == MVICP_NN_GRID;
  h.last_rms = -1.0;   // consumed: only a solve that follows THIS search may predict the next one
  // only the grid kernel and the tile kernel's BND build leave the per-query lower bounds the temporal cache needs; the cutoff must
  // not change either
  h.nn_cache_valid = ((p.method == MVICP_NN_GRID) && !opt.nn_tree_only && !opt.nn_skip_far) || p.tile_lb;
  h.nn_cache_thresh = in.thresh;
  h.auto_last_method = p.handed_over ? MVICP_NN_GRID : p.method;   // (the policy's "already handed over" state)
  h.nn_cache_edge.assign(p.active, p.active + in.E);
  for (int e = 0; e < in.E; ++e) { h.list_valid[e] = p.active[e]; if (in.owned[e]) h.qpos_valid[e] = p.active[e]; if (p.active[e]) h.explicit_list[e] = 0; }
}

// 3. What arrived after the wait.  tie_word / far_word: what this search's tie fix-up / far launch reported (1 = unknown).  res = (count,
// median d2) x E | armed, scales = the SoftLOne scales the device derived (read only when the plan armed): of this rank's edges with a single
// rank, summed over the ranks with an exchange.  redone: a median had left its bracket and the full select ran again (the queued evaluation
// used the scales of the failed select).  -> the queued first evaluation may be used.
inline bool record_arrived(const SearchInputs& in, const SearchPlan& p, SearchHistory& h, unsigned int tie_word, unsigned int far_word, const double* res,
                           const double* scales, bool redone) {
  const int E = in.E;
  // a skipped launch keeps last search's zero: the next search's skip decisions
  if (p.tie_launched) h.corr_tie_seen = tie_word;
  if (p.far_launched) h.corr_far_seen = far_word;
  else if (p.method != MVICP_NN_GRID) h.corr_far_seen = 1u;
  // trust the queued evaluation only if (i) every rank queued one, and (ii) the scales the device derived from the medians are the
  // host's (IEEE sqrt) bit for bit — checked on ALL edges from exchanged data, so every rank reaches the same verdict
  bool spec_bad = redone;
  if (p.spec_arm && res[2 * (size_t)E] != (double)(in.exchange ? in.world : 1)) spec_bad = true;
  for (int e = 0; e < E; ++e) {
    const bool mine = in.owned[e] && p.active[e];
    // (count, median d2): weight = (float)(1.5 * sqrt(median d2))  (frame.cpp:168-176)
    const double cnt = (in.exchange || mine) ? res[2 * e] : 0.0, med = cnt > 0 ? res[2 * e + 1] : 0.0;
    if (!(in.exchange ? !p.src_fixed[e] : mine)) h.sel_med1[e] = h.sel_med2[e] = -1.0;   // (exchanged: every searched edge's median is known here)
    else { h.sel_med2[e] = h.sel_med1[e]; h.sel_med1[e] = cnt > 0 ? med : -1.0; }
    if (p.spec_arm && !spec_bad && (in.exchange || mine)) {
      const double a_host = cnt > 0 ? (double)(float)(std::sqrt(med) * 1.5) : 0.0;
      if (scales[e] != a_host) spec_bad = true;
    }
    h.h_count[e] = (int)cnt;
    h.h_weight[e] = h.h_count[e] > 0 ? (float)(std::sqrt(med) * 1.5) : 0.f;
  }
  if (!p.sel_skip) h.sel_result_armed = p.spec_arm;   // (a skipped select leaves d_a and its mapped copy as they were)
  h.sel_result_valid = !in.exchange;
  h.have_corr = true;
  return p.spec_arm && !spec_bad;
}

}  // namespace mvicp
