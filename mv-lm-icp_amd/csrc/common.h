// Internal declarations shared by the HIP translation units of libmvicp_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <future>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mvicp.h"
#include "abi_guard.h"
#include "search_plan.h"   // host-only: the search policy, its options and history, the layout of the per-edge transform block

namespace mvicp {

void set_error(const char* fmt, ...);

#define MV_HIP(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      mvicp::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));  \
      return MVICP_ERR_HIP;                                                                   \
    }                                                                                         \
  } while (0)

#define MV_CHECK(call)            \
  do {                            \
    int _s = (call);              \
    if (_s != MVICP_OK) return _s; \
  } while (0)

constexpr int kLinPartial = 32;      // doubles per linearize workgroup partial (28 plane / 29 point, padded)
constexpr int kLinThreads = 256;
constexpr int kCompactBlock = 1024;  // queries per compaction workgroup
constexpr int kSelBlock = 8192;      // keys per radix-select workgroup
constexpr int kEdgeRel = 12;         // R_ds(9, column-major) t_ds(3)

// Uniform grid (spatial hash) over one cloud; see nn_grid.hip.
struct GridDev {
  int dims[3] = {0, 0, 0};
  double origin[3] = {0, 0, 0};
  double cell = 0.0, inv_cell = 0.0;
  int n_cells = 0;             // occupied cells
  double* spts = nullptr;      // n x 3 in the cloud's sorted order (balanced k-d order by default, ctx::grid_curve)
  int* sidx = nullptr;         // n: original index of sorted point
  void* srec = nullptr;        // n x 32 B {x, y, z, idx}: the same, packed for the per-lane candidate scans
  void* crec = nullptr;        // the records in hash-CELL order ({start, count} runs of `table`); aliases srec unless grid_curve = 2
  double* snor = nullptr;      // n x 3 normals in sorted order (null without normals)
  // reject mask (mvicp_set_reject_mask): n bytes, nonzero = pairs with this point are dropped by the search's acceptance test.  smask in
  // sorted order (what the kernels index), omask the caller's bytes in original order (the read-back); mask_roles = MVICP_REJECT_AS_* bits,
  // 0 = no mask (the buffers may stay allocated).  Lives and dies with the cloud, like snor
  unsigned char* smask = nullptr; unsigned char* omask = nullptr; int mask_roles = 0;
  int* inv = nullptr;          // n: original index -> sorted position
  std::vector<int> h_order, h_inv;  // host copies: sorted -> original, original -> sorted
  void* table = nullptr;       // open-addressing hash: cell -> (start, count), 16-B entries
  unsigned int table_mask = 0; int table_shift = 0;
  float* oct = nullptr;        // implicit complete 8-ary box tree, 8 floats per node {lo.xyz, hi.xyz, pad2}
  int oct_leaf = 0; long long oct_first_leaf = 0;
  // 64-wide box hierarchy over the same sorted array (nn_tile.hip): level 0 = boxes of 64-point leaves,
  // level l+1 = boxes of 64 consecutive level-l boxes; SoA per level: 6 arrays of `wide_cnt[l]` floats.
  float* wide = nullptr;
  double maxabs = 0.0;         // largest |coordinate|
  int wide_levels = 0;
  int wide_cnt[6] = {0, 0, 0, 0, 0, 0};
  long long wide_off[6] = {0, 0, 0, 0, 0, 0};
  // matrix-pipe operands (nn_mfma.hip, build_mfma): per 32-point tile 64 x 16 B of ready-made v_mfma_f32_32x32x16_f16 A fragments, per block of
  // 64 tiles the origin / scale / error terms they refer to
  void* mf_ops = nullptr; void* mf_blk = nullptr;
  double struct_bytes = 0.0;
  // dense brick map over the cells (nn_grid.hip, nn_cell_kernel): brick = 4x4x4 cells -> {occupancy mask, row of the cell table};
  // cell table row = 64 x {start, count} of the cell runs in the sorted array.  Null when the grid is too large for a dense map.
  void* bricks = nullptr; void* celltab = nullptr; int bdims[3] = {0, 0, 0};
  size_t celltab_bytes = 0;    // bytes of the cell table in use
  // overlap census (overlap.hip): the sorted positions of the cloud's `ov_samp_s` sample points, ascending; built on first use for
  // a given max_samples and kept until it changes (null: none yet, or every point is a sample)
  int* ov_samp = nullptr; int ov_samp_s = 0;
};

struct PointRec { double x, y, z; long long idx; };  // 32-B aligned sorted point + original index

// The per-cloud structure build of one mvicp_set_frame, running on a host thread of its own (api.cpp): the call returns once the cloud is
// on the device, the k-d order / box hierarchy / matrix-pipe operands / hash are built behind it, one cloud beside the other, and every
// entry point that needs a structure waits for the pending builds first (finish_builds).
struct BuildJob { std::future<int> fut; std::string err; std::vector<double> xyz, nrm; };

// What the device build needs from the one reduction mvicp_set_frame_device runs before it returns (build.hip device_bounds)
struct DevBounds { double lo[3], hi[3], max_norm, maxabs, wall_ms; int nonfinite, pad; };

struct FrameDev {
  std::shared_ptr<BuildJob> job;   // pending structure build (null: none)
  std::string build_error;         // sticky: this cloud's structure build failed (message); cleared only by a new mvicp_set_frame of this slot.  While it
                                   // is set, every entry point that needs the structures fails — never a silent O(N^2) brute-force fallback
  int n = 0;
  double* pts = nullptr;  // n x 3 AoS, original order
  double* nor = nullptr;  // n x 3 or null
  GridDev grid;
  bool has_grid = false;
  double max_norm = 0.0;   // max |p| over the cloud (bounds how far a pose change can move a query)
  double build_ms[2] = {0.0, -1.0};   // the last structure build of this slot: host wall ms (upload excluded), device ms of the device build (-1: host build)
  // the reference's own tree over this cloud (kdvisit.h: split structure of nanoflann's buildIndex, leaf_max_size 1): decides exact distance
  // ties the way the reference does (nn_tie.hip) and orders the k-NN lists of the normals (normals.hip); built on first use
  void* tie_nodes = nullptr; int* tie_ord = nullptr; int* tie_slot = nullptr; double tie_box[6] = {0, 0, 0, 0, 0, 0}; bool has_tie = false; int tie_levels = 0;   // tie_levels: levels of the tree (build_visit_tree)
};

// the frame's reject mask in sorted order when it applies in `role` (one MVICP_REJECT_AS_* bit), else null
inline const unsigned char* reject_mask_of(const FrameDev& f, int role) { return (f.grid.mask_roles & role) ? f.grid.smask : nullptr; }

struct ProfEntry {
  double ms = 0.0;
  long long launches = 0;
  double bytes = 0.0;          // the library's own byte model of the scope's launches
  double survey_bytes = 0.0;   // NN scopes: SURVEY.md 8(d) algorithmic bytes (36 B/query + 24 B/candidate point fetched + 8 B/box or cell looked up)
  double queries = 0.0;        // NN scopes: queries answered
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<hipEvent_t> pool;
};

// ---- buffers and results a stage of the library owns ---------------------------------------------------------------------------------
// A stage (voxel grid, outlier filter, neighbour search, FPFH, descriptor matching, consensus, batched coarse poses, ISS keypoints, estimated
// normals, oriented normals, clusters, the dominant plane, boundary points) keeps its LAST result on the context until the caller has fetched it.  Ownership, stated once for all thirteen: the stage's struct below holds
// buffers of its own (so that a call touches nothing a search, a queued evaluation, the census or another stage uses), kept between
// calls and grown on demand, the result arrays as views into them, and the sizes / flags, whose defaults mean "no result".  A call marks
// its result as gone when it starts (a failed call leaves none behind) and sets it after its last wait; the result then lives until the
// stage's next call, mvicp_set_num_frames or mvicp_destroy, and the last two release every stage through release_stages (api.cpp):
// release() frees the buffers and assigns a default-constructed struct, so no view, size or flag can outlive them.  The five stages that
// end by selecting rows of a stored cloud (outlier filter, ISS keypoints, clusters, the dominant plane, boundary points) keep those rows in
// a RowSelection of their own, `sel`, which follows the same rules inside the stage: reserved by the stage call, dropped and released with it.

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int grid_of(long long n, int threads) { return (int)((n + threads - 1) / threads); }

// growable device buffer: reserve keeps a buffer that is large enough, else frees it and allocates exactly `need` (the contents are lost)
struct DevBuf {
  char* p = nullptr; size_t cap = 0;
  int reserve(size_t need) {
    if (need <= cap) return MVICP_OK;
    if (p) MV_HIP(hipFree(p));
    p = nullptr; cap = 0;
    MV_HIP(hipMalloc((void**)&p, need));
    cap = need;
    return MVICP_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
// the same in pinned host memory
struct PinBuf {
  char* p = nullptr; size_t cap = 0;
  int reserve(size_t need) {
    if (need <= cap) return MVICP_OK;
    if (p) MV_HIP(hipHostFree(p));
    p = nullptr; cap = 0;
    MV_HIP(hipHostMalloc((void**)&p, need, hipHostMallocDefault));
    cap = need;
    return MVICP_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// row_select.hip.  The rows a stage selects from a stored cloud, in ascending original index: the one owner of where they live, how they are
// produced (select_rows, row_select.h) and when they carry normals.  dev: [kept word | flag | rank | xyz | nrm | idx | klabel, when labels were
// asked for], tmp: rocprim storage of the scan, pin: the kept word's host copy.  A stage that selects rows holds one as `sel`; the stage call
// reserves it (so that a selection allocates nothing), the stage's drop_result() / release() end it.  has_normals: the frame had stored normals
// WHEN THE SELECTION RAN -- the rule for all five stages; normals that arrive later (an adopt) are in the next selection, not in this one
struct RowSelection {
  DevBuf dev, tmp; PinBuf pin;
  int* flag = nullptr; int* rank = nullptr; double* xyz = nullptr; double* nrm = nullptr; int* idx = nullptr; int* klabel = nullptr;
  long long rows = -1, kept = -1; int has_normals = 0;   // rows reserved for (< 0: none), rows of the last selection (< 0: none)
  int reserve(long long n, bool labels, hipStream_t stream);   // row_select.hip (asks rocprim for the scan's storage); ends the last selection
  void drop() { kept = -1; has_normals = 0; }
  void release() { dev.release(); tmp.release(); pin.release(); *this = RowSelection(); }
};

// voxel.hip.  The result is three allocations of its own, made once the voxel count is known and freed at the start of the next call
// (drop_result); growable are the scratch, the rocprim storage and the pinned control block
struct VoxelStage {
  DevBuf scratch, tmp; PinBuf pin;
  double* xyz = nullptr; double* nrm = nullptr; int* cnt = nullptr; long long m = -1; int has_normals = 0;   // m < 0: none
  void drop_result() {
    if (xyz) (void)hipFree(xyz);
    if (nrm) (void)hipFree(nrm);
    if (cnt) (void)hipFree(cnt);
    xyz = nullptr; nrm = nullptr; cnt = nullptr; m = -1; has_normals = 0;
  }
  void release() { drop_result(); scratch.release(); tmp.release(); pin.release(); *this = VoxelStage(); }
};
// outlier.hip.  dev: one arena [control | mdist | kd2], pin: the control block's host copy, sel: the rows kept
struct OutlierStage {
  DevBuf dev; PinBuf pin; RowSelection sel;
  double* mdist = nullptr; double* kd2 = nullptr;
  long long n = -1;   // n < 0: none
  void release() { dev.release(); pin.release(); sel.release(); *this = OutlierStage(); }
};
// knn.hip.  dev holds [control | cnt | off], ent the entries [idx | d2] (all mode: behind them the same in visiting order), tmp the
// scratch (staged host queries, sort keys, rocprim storage), pin the control block's host copy
struct KnnStage {
  DevBuf dev, ent, tmp; PinBuf pin;
  int* cnt = nullptr; long long* off = nullptr; int* idx = nullptr; double* d2 = nullptr;
  long long m = -1, total = 0; int k = 0;   // rows (< 0: none), entries over all rows, the k of the call (0: all mode, CSR)
  void release() { dev.release(); ent.release(); tmp.release(); pin.release(); *this = KnnStage(); }
};
// fpfh.hip.  dev: [desc n x 33 doubles | used n ints | SPFH records n x 48 B]; the neighbourhoods are the KnnStage result of the search
// the call runs, so there is no second set of search buffers
struct FpfhStage {
  DevBuf dev;
  double* desc = nullptr; int* used = nullptr;
  long long rows = -1;   // < 0: none
  void release() { dev.release(); *this = FpfhStage(); }
};
// match.hip.  dev holds [fwd_idx | fwd_d2 | bwd_idx | bwd_d2 | flag], tmp the scratch (staged host operands, the per-chunk partial lists)
struct MatchStage {
  DevBuf dev, tmp;
  int* fwd_idx = nullptr; int* bwd_idx = nullptr; double* fwd_d2 = nullptr; double* bwd_d2 = nullptr;
  long long m = -1, n = -1;   // m < 0: none
  void release() { dev.release(); tmp.release(); *this = MatchStage(); }
};
// consensus.hip.  dev: [control | count H ints | accepted h | flags c bytes | staged host pairs]
struct ConsensusStage {
  DevBuf dev;
  int* count = nullptr; unsigned char* flags = nullptr;
  long long H = -1, c = -1;   // H < 0: none
  void release() { dev.release(); *this = ConsensusStage(); }
};
// coarse.hip.  dev holds [pairs | flags] in per-edge segments (edge e: seg[e], cnt[e] pairs), tmp the scratch of a call, work the
// scoring work table
struct CoarseStage {
  DevBuf dev, tmp, work;
  int* pairs = nullptr; unsigned char* flags = nullptr;
  std::vector<long long> seg; std::vector<int> cnt;
  int edges = -1;   // < 0: none
  void release() { dev.release(); tmp.release(); work.release(); *this = CoarseStage(); }
};
// iss.hip.  dev: one arena [control | saliency | cnt_salient | cnt_nms], pin: the control block's host copy, sel: the keypoints' rows (sel.kept
// = their number)
struct IssStage {
  DevBuf dev; PinBuf pin; RowSelection sel;
  double* sal = nullptr; int* cnt_s = nullptr; int* cnt_n = nullptr;
  long long n = -1;   // points of the frame (< 0: none)
  void release() { dev.release(); pin.release(); sel.release(); *this = IssStage(); }
};
// normals_pca.hip, normals_jet.hip, smooth.hip.  dev: [nrm n x 3 doubles | curvature n doubles | used n ints | fitted n bytes, after mvicp_fit_normals only];
// the neighbourhoods are the KnnStage result of the search the call runs.  frame: the slot the result was computed for (mvicp_normals_adopt
// writes there); an upload to that slot drops the result.  has_fit: the result is mvicp_fit_normals' or mvicp_smooth_points'
// (mvicp_normals_fit_fetch serves it).  smooth.hip adds smo: [xyz n x 3 doubles | shift | H | K n doubles each | moved n bytes], the part of
// a mvicp_smooth_points result that mvicp_smooth_fetch serves (has_smooth); it lives and ends with the rest of the result
struct NormalsStage {
  DevBuf dev, smo;
  double* nrm = nullptr; double* curv = nullptr; int* used = nullptr; unsigned char* fitted = nullptr;
  double* xyz = nullptr; double* shift = nullptr; double* H = nullptr; double* K = nullptr; unsigned char* moved = nullptr;
  long long rows = -1; int frame = -1, has_fit = 0, has_smooth = 0;   // rows < 0: none
  void drop_result() { rows = -1; frame = -1; has_fit = 0; has_smooth = 0; }
  // the layout of dev for a result of N rows with the fitted bytes
  int reserve_fit(size_t N) {
    const size_t off_curv = align256(24 * N), off_used = off_curv + align256(8 * N), off_fit = off_used + align256(4 * N);
    MV_CHECK(dev.reserve(off_fit + align256(N)));
    nrm = reinterpret_cast<double*>(dev.p); curv = reinterpret_cast<double*>(dev.p + off_curv);
    used = reinterpret_cast<int*>(dev.p + off_used); fitted = reinterpret_cast<unsigned char*>(dev.p + off_fit);
    return MVICP_OK;
  }
  void release() { dev.release(); smo.release(); *this = NormalsStage(); }
};

// orient.hip.  dev: [nrm n x 3 doubles | comp n ints | flip n bytes | the work arrays of the Boruvka rounds], pin: the counters the host
// reads per round; the neighbourhoods are the KnnStage result of the search the call runs.  frame: the slot the result was computed for
// (mvicp_orient_adopt writes there); an upload to that slot drops the result
struct OrientStage {
  DevBuf dev; PinBuf pin;
  double* nrm = nullptr; unsigned char* flip = nullptr; int* comp = nullptr;
  long long rows = -1, comps = 0; int frame = -1;   // rows < 0: none
  void drop_result() { rows = -1; comps = 0; frame = -1; }
  void release() { dev.release(); pin.release(); *this = OrientStage(); }
};
// cluster.hip.  dev: one arena [control | core | parent | root | root flag | root rank | label | size | keep], tmp: rocprim storage of the label
// pass's scan, pin: the host copy of [control | size, later the keep bytes]; h_size: the cluster sizes for the select rule.  frame: the slot
// the result was computed for (mvicp_cluster_select reads its stored rows); an upload to that slot drops the result.  sel: the rows of the
// last mvicp_cluster_select of this result, with their labels
struct ClusterStage {
  DevBuf dev, tmp; PinBuf pin; RowSelection sel;
  int* label = nullptr; unsigned char* core = nullptr; int* size = nullptr; unsigned char* keep = nullptr;   // keep: a byte per cluster, the last select rule's
  std::vector<int> h_size;
  long long n = -1, clusters = -1; int frame = -1;   // n < 0: none
  void drop_result() { n = -1; clusters = -1; frame = -1; h_size.clear(); sel.drop(); }
  void release() { dev.release(); tmp.release(); pin.release(); sel.release(); *this = ClusterStage(); }
};
// plane.hip.  dev: one arena [control | count | accepted h | flags], pin: the host copy of the control block.  frame: the slot the result was
// computed for (mvicp_plane_select reads its stored rows); an upload to that slot drops the result.  sel: the rows of the last
// mvicp_plane_select of this result
struct PlaneStage {
  DevBuf dev; PinBuf pin; RowSelection sel;
  int* count = nullptr; unsigned char* flags = nullptr;
  long long n = -1, H = -1; int frame = -1;   // n < 0: none
  void drop_result() { n = -1; H = -1; frame = -1; sel.drop(); }
  void release() { dev.release(); pin.release(); sel.release(); *this = PlaneStage(); }
};
// boundary.hip.  dev: one arena [control | flag bytes | open | valid | used], pin: the host copy of the control block.  frame: the slot the
// result was computed for (mvicp_boundary_select reads its stored rows); an upload to that slot drops the result.  sel: the rows of the
// last mvicp_boundary_select of this result
struct BoundaryStage {
  DevBuf dev; PinBuf pin; RowSelection sel;
  unsigned char* flag = nullptr; int* open = nullptr; int* valid = nullptr; int* used = nullptr;
  long long n = -1; int frame = -1;   // n < 0: none
  void drop_result() { n = -1; frame = -1; sel.drop(); }
  void release() { dev.release(); pin.release(); sel.release(); *this = BoundaryStage(); }
};
// orient.hip (mvicp_normal_agreement).  dev: [poses | per-edge pointer tables | per-edge counts | pos | neg], pin: the host copy of pos | neg
struct AgreementStage {
  DevBuf dev; PinBuf pin;
  void release() { dev.release(); pin.release(); *this = AgreementStage(); }
};

struct RcclApi;  // comm.cpp

}  // namespace mvicp

struct mvicp_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int n_frames = 0;
  std::vector<mvicp::FrameDev> frames;

  // the search policy's options, cross-round state and per-call plan (search_plan.h; api.cpp correspond_once executes the plan)
  mvicp::SearchOptions opt;
  mvicp::SearchHistory hist;
  mvicp::SearchPlan plan;
  std::vector<mvicp::PlanFrame> plan_frames;   // n_frames: what the policy reads of the clouds, refreshed by every search

  // graph + sharding
  int rank = 0, world = 1;
  int E = 0;
  std::vector<int> esrc, edst;
  std::vector<char> owned;         // E
  std::vector<long long> cap_off;  // E+1: prefix of N_src over OWNED edges (0-width for others)
  long long total_cap = 0;

  // device per-edge tables.  d_xf / d_nsrc / d_dirty and d_rel / d_a are views into ONE control block (d_ctl) mirrored in
  // pinned host memory, so a round costs one upload before the NN stage and one per LM evaluation:
  //   region 1 (correspond): xf [E x kEdgeXf] | nsrc [E int] | dirty [E int]        region 2 (evaluate): rel [E x kEdgeRel] | a [E]
  // Between the two lies rel2 [E x kEdgeRel], the second pose set of a paired evaluation (linearize.hip): a search that queues evaluations uploads
  // region 1 | rel2 | rel in one copy (the scales `a` behind them are written on the device).
  double* d_ctl = nullptr; size_t ctl_r1 = 0, ctl_rel2_off = 0, ctl_r2_off = 0, ctl_r2 = 0;   // sizes / offsets in doubles
  int* d_esrc = nullptr; int* d_edst = nullptr;
  long long* d_cap_off = nullptr;   // E+1
  int* d_nsrc = nullptr;            // E: N_src if owned and active else 0
  int* d_count = nullptr;           // E
  double* d_a = nullptr;            // E: SoftLOne scale (double)(float)weight
  double* d_xf = nullptr;           // E x kEdgeXf
  double* d_rel = nullptr;          // E x kEdgeRel
  double* d_rel2 = nullptr;         // E x kEdgeRel: relative transforms of the second pose set of a paired launch
  // per-query (total_cap)
  int* d_nn_idx = nullptr; double* d_nn_d2 = nullptr;
  float* d_nn_lb = nullptr;         // fp32, rounded down: lower bound on the DISTANCE from the query to every target other than nn_idx (temporal cache)
  // per-correspondence (total_cap)
  int* d_first = nullptr; int* d_second = nullptr; double* d_cd2 = nullptr;
  int* d_qpos = nullptr;            // per query: its position in the edge's compacted list, or -1 (rejected by the cutoff or by a reject mask)
  int* d_dirty = nullptr;           // E: != 0 -> the edge's list (membership or a neighbour) changed this round: re-compact + re-gather
  int* d_dirty_slots = nullptr; int* d_dslot_off = nullptr; std::vector<int> dslot_off; int n_dslots = 0;  // one slot per 256 queries
  // the lists in the reference's layout (export.hip): {first, second, dist} triples, ascending first, all exportable edges of the last search
  void* d_export = nullptr; void* h_export = nullptr; size_t export_cap = 0;   // device staging / pinned host copy (capacity in triples)
  int* d_xblock_cnt = nullptr;
  std::vector<long long> export_off; // E+1: edge e's triples = h_export[export_off[e] .. export_off[e + 1])
  bool export_valid = false;         // h_export holds the lists as they are on the device now
  // the copy of the export into pinned memory goes in CHUNKS (one per run of edges with the same source frame), each followed by an event, so that a
  // caller that fills its lists frame by frame (host/frame.cpp) slices frame i while frames i+1.. are still on the bus (mvicp_map_correspondences_async)
  std::vector<hipEvent_t> export_events; std::vector<int> export_edge_chunk; int export_chunks = 0; bool export_in_flight = false;
  std::vector<unsigned long long> corr_epoch;   // E: changes whenever the edge's list (count, triples, weight) may differ from what it was (mvicp_correspondence_epochs)
  unsigned long long epoch_counter = 0;
  double* d_stream = nullptr;       // 10 x total_cap SoA: p (3) | n (3) | c = n . q | q (3)   (linearize.hip)
  // compaction scratch
  int n_cblocks = 0;                // total compaction blocks over owned edges
  std::vector<int> cblock_off;      // E+1
  int* d_cblock_off = nullptr; int* d_cblock_cnt = nullptr;
  // select scratch
  unsigned int* d_sel_hist = nullptr;   // cnt_lt [E] | cnt_mid [E] | hist [E][2048]: every kernel re-zeroes what it used (no memset in a search)
  double* d_median = nullptr;
  int n_sblocks = 0; std::vector<int> sblock_off; int* d_sblock_off = nullptr;   // kSelBlock keys per workgroup
  double* d_sel_lohi = nullptr;      // view into the control block: per edge the bracket [lo, hi] (d2) of the one-pass select
  bool sel_scratch_clean = false;    // d_sel_hist is all zero on the device: after mvicp_set_graph's memset and after every search that returned OK
  double* d_sel_keys1 = nullptr;     // compact key buffer of the bracket pass (total_cap)
  // linearize chunks
  bool lin_interleave = true;       // launch order of the linearize workgroups: chunks of the edges that share a source cloud interleaved in groups of 8 (api.cpp mvicp_set_graph)
  bool lin_tail_last = true;        // ... and every edge's partial last chunk behind all full chunks: the workgroups that start last are the short ones (api.cpp mvicp_set_graph)
  bool lin_share_p = true;          // linearize reads p from the sorted source cloud when an edge's list is the identity (option "lin_share_p")
  int lin_chunk_override = 0;
  int lin_chunk = 4096;             // correspondences per linearize workgroup (chosen from the GLOBAL problem size)
  int n_chunks = 0;                 // chunks = slots of the partials
  int n_lin_wg = 0;                 // entries of the launch table = workgroups of a launch (>= n_chunks: the table may hold pads)
  std::vector<int> chunk_first;     // E+1
  int* d_chunk_edge = nullptr; int* d_chunk_start = nullptr; int* d_chunk_first = nullptr;
  double* d_partials = nullptr;     // 2 x n_chunks x kLinPartial (second half: the second pose set of a paired launch)
  double gicp_eps = 1e-3;           // the epsilon of the plane-to-plane evaluation under way (mvicp_linearize_gicp / mvicp_optimize_gicp set it before evaluate_blocks(kMetricGicp))
  mvicp::PinBuf sym_lo_pin; mvicp::DevBuf sym_lo_dev;   // E x kEdgeRel doubles: low parts of the relative transforms of a symmetric evaluation (api.cpp upload_rel_sym,
                                    // linearize_sym.hip); buffers of their own, allocated by the first symmetric evaluation of a graph, released with the graph
  double* d_out = nullptr;          // E x 91 blocks | E x 2 (count, median d2) | 1 "armed" slot: ONE buffer, so that with N > 1 ranks a round's
                                    // counts / medians / use-the-queued-evaluation decision travel in the same all-reduce as the queued blocks
  double* d_res_target = nullptr;   // where the select kernels put (count, median d2): null = mapped host memory (single rank), else d_out's tail
  // pinned (device-mapped) host staging: [control-block mirror | blocks E x 91 | results E x 2 | misc]
  double* h_pin = nullptr; size_t h_pin_doubles = 0;
  size_t pin_blocks_off = 0, pin_res_off = 0, pin_misc_off = 0;
  double* d_res_host = nullptr;     // device view of the results region: (count, median d2) per edge, written by bracket_final_kernel
  double* d_blocks_host = nullptr;  // device view of the blocks region: single-rank evaluations write the E x 91 blocks straight to the host
  double* lin_out = nullptr;        // where the next launch_linearize puts the E x 91 blocks (d_out or d_blocks_host)
  // Speculative first evaluation: mvicp_correspond queues the linearization the NEXT mvicp_optimize will ask for first (same poses,
  // the parameterization / cost flags of the previous solve) right behind the select kernels, so the round waits once for
  // (counts, medians, first blocks) instead of twice.  Used only if the solve really asks for exactly that evaluation.
  int spec_q_plane = 0, spec_q_robust = 0;   // flags the QUEUED evaluation was launched with (spec_plane / spec_robust may have moved on since)
  bool spec_arm = false;            // this correspond call queues one (select kernels write the SoftLOne scales on the device)
  bool spec_ready = false;          // blocks of spec_poses are in the pinned spec region
  std::vector<double> spec_poses;   // n_frames x 16: poses the speculative evaluation was made at (after the parameterization round trip)
  size_t pin_spec_off = 0, pin_adev_off = 0; double* d_spec_host = nullptr; double* d_adev_host = nullptr;
  // Second queued evaluation (round 6, single rank).  At the fixed point of a registration every round's solve is: first evaluation (queued, above) -> one LM
  // iteration -> candidate evaluation -> function-tolerance stop, and the candidate poses are last round's bit for bit (same inputs).  When this search's poses
  // are bit-identical to the last search's, the candidate evaluation of the LAST solve is queued right behind the first one (relative transforms from a second
  // pinned slice, copied into d_rel in stream order between the two — or, option lin_pair, both in ONE paired launch that reads the operand stream once, with
  // the second set of relative transforms riding on the control-block upload), so the round waits ONCE for both.  Used only if the solve really asks for exactly those
  // poses; nothing is skipped — the work is queued earlier.
  bool spec2_armed = false, spec2_ready = false; int spec2_plane = 0, spec2_robust = 0;
  std::vector<double> spec2_poses;       // poses the second queued evaluation was made at
  size_t pin_spec2_off = 0, pin_rel2_off = 0; double* d_spec2_host = nullptr;
  size_t pin_blocks2_off = 0; double* d_blocks2_host = nullptr;   // second block set of mvicp_linearize_pair (device view of its pinned region)
  double* d_a_check = nullptr;      // where this search's select kernels copy the SoftLOne scales they derive: mapped host memory (single rank) or d_out's tail
  bool spin_wait = false;           // poll the stream instead of a blocking wait (measured: no gain, HIP's own wait already spins)
  unsigned long long* h_census = nullptr;   // pinned: 8 counters of the last NN launch, resolved after the round's own sync
  bool census_pending = false; double census_nq = 0; int census_kind = 0; const char* census_scope = "nn_grid";   // kind: 0 grid (per-lane), 1 tree-only grid, 2 tile, 3 grid (cell staging)
  // brute-force split scratch
  int* d_split_idx = nullptr; double* d_split_d2 = nullptr; size_t split_cap = 0;

  // overlap census (overlap.hip): buffers of its own — [jobs | item offsets | hits | sumq] on the device and the same in pinned host
  // memory — so that mvicp_overlap touches nothing a search, a queued evaluation or the shared control block uses
  char* ov_dev = nullptr; char* ov_pin = nullptr; size_t ov_bytes = 0;

  // the library-owned results (the *Stage structs above): one struct per stage; the options that sit between them are settings and outlive a result
  mvicp::VoxelStage vox;
  int voxel_permute = 1;           // option "voxel_permute": lay w / R n out in sorted order before the reduction (0: the reduction re-gathers through seq)
  mvicp::OutlierStage out;
  mvicp::KnnStage knn;
  int knn_order = 1;               // option "knn_order": queries are answered in the order of their home cells (0: as given); the result is the same bytes
  mvicp::FpfhStage fpfh;
  mvicp::MatchStage match;
  int match_chunk = 2048;          // option "match_chunk": rows of the right operand per blockIdx.y chunk; the result is the same bytes
  mvicp::ConsensusStage cons;
  mvicp::CoarseStage coarse;
  mvicp::IssStage iss;
  mvicp::NormalsStage nrm;
  mvicp::OrientStage ori;
  mvicp::AgreementStage agree;
  mvicp::ClusterStage clu;
  mvicp::PlaneStage plane;
  mvicp::BoundaryStage bnd;
  std::vector<char> src_fixed;     // E: the edge's source frame was fixed in the last mvicp_correspond (0 before the first): mvicp_normal_agreement skips it

  // cached small tables
  struct CachedTable { std::vector<char> bytes; void* d = nullptr; size_t cap = 0; };
  std::map<std::string, CachedTable> tables;
  // table scratch
  char* d_scratch = nullptr; size_t scratch_bytes = 0, scratch_used = 0;
  std::vector<char> active;        // E: owned && src not fixed (set by correspond)

  // comm
  mvicp::RcclApi* rccl = nullptr;
  void* comm = nullptr;
  mvicp_allreduce_fn ar_fn = nullptr; void* ar_user = nullptr;   // host-staged all-reduce supplied by the launcher (no RCCL)
  std::vector<double> ar_host;

  bool async_build = true;          // option "async_build": mvicp_set_frame builds the per-cloud structures on a background host thread
  std::atomic<int> fault_inject_build{0};   // tests only: the n-th structure build from now fails (builds run on background threads)
  int fault_inject = 0, fault_inject_eval = 0;   // tests only: make the n-th search / exchanged evaluation from now fail locally before its collective
  // options / NN census (profiling only)
  bool nn_census = false;          // count candidates / tree nodes per launch while profiling (small extra cost)
  void* d_census = nullptr; size_t census_bytes = 0;
  void* d_far_list = nullptr; size_t far_cap = 0; unsigned int* d_far_count = nullptr;  // nn_grid far-query list
  int far_parity = 0;              // d_far_count holds TWO counters used alternately; a launch zeroes the one the next launch will use
  unsigned int* h_far_seen = nullptr; unsigned int* d_far_seen = nullptr;   // mapped host word: far-list length of the last nn_far_kernel launch
  double nn_search_factor = 4.0;   // the kernels look for a neighbour within this many cutoffs (0 = unbounded, like the reference's findNeighbors): a query the
                                   // cutoff rejects then still has a neighbour to seed next round's search with and a temporal-cache bound, instead of being
                                   // searched from scratch every round (partial overlap: a third of the queries); the filter of frame.cpp:156 is applied after
  unsigned long long* d_tie_list = nullptr; size_t tie_cap = 0; unsigned int* d_tie_count = nullptr; int tie_parity = 0;   // queries reported by the NN kernels
  void* d_tie_deep = nullptr; size_t tie_deep_bytes = 0;   // per-lane walk stacks of nn_tie_deep_kernel (targets whose tree has more levels than the per-lane array)
  unsigned int* h_tie_seen = nullptr; unsigned int* d_tie_seen = nullptr;   // mapped host word: reports of the last fix-up launch (read after the round's wait)
  bool tile_seed = true;           // tile kernel starts from last round's neighbours when there are any
  bool reject_cache = true;        // cache-aware rounds: "provably still rejected by the cutoff" counts as a temporal-cache hit (nn_tile.hip / nn_mfma.hip prologue)
  int tile_miss = 8;               // cache-aware rounds: waves with at most this many missed lanes use nn_tile.hip's miss_block (0 = off)
  double mfma_kacc = 34.0;         // nn_mfma.hip: allowance for the fp32 accumulation inside one matrix instruction, in units of 2^-24 x sum |terms| (see tau_pieces)
  int mfma_lbt = 1;                // nn_mfma.hip: unseeded launches test every tile's box per lane before screening it (scan_block LBT)
  int mfma_entry = 0;              // nn_mfma.hip experiment (round 6): seeded launches enter at the seeds' blocks + one flat sweep over the block boxes instead of the top-down walk
  int mfma_trig = 2;               // nn_mfma.hip: a lane with more than this many screen hits in a tile triggers the nearest-first second screen
  int tile_waves = 0;              // nn_tile_kernel variant: waves per SIMD it is compiled for (0 = the measured best for the depth)
  double prune_rho = 0.05;         // grid kernel: with a seed, skip block cells farther than seed distance + prune_rho * cell edge; 0 = off
  int grid_curve = 2;              // order of the sorted clouds: 0 Morton (Z-order) of the cells, 1 Hilbert of the cells, 2 balanced k-d order
  double grid_target = 5.0;        // points per occupied cell the cell-edge heuristic aims at (4-6 measure the same within 2 %)
  double nn_candidates = 0, nn_nodes = 0, nn_far = 0, nn_queries = 0, nn_hits = 0, nn_fetched = 0;
  double nn_dbg[4] = {0, 0, 0, 0};   // nn_mfma_kernel census: second-screen passes, confirmation rounds, blocks scanned (all per wave), fp64 confirmations (per lane)
  char last_nn_launch[48] = "";      // which NN kernel instantiation the last search launched (mvicp_last_nn_launch): written by the launchers, "" before the first

  // profiling
  bool profile = false; int profile_level = 0;   // 1: every scope, 2: only "nn" and "linearize"
  std::map<std::string, mvicp::ProfEntry> prof;
};

namespace mvicp {

// kernels (each defined in its own TU)
int launch_nn_brute_edges(mvicp_ctx* c);                                             // nn_brute.hip
int launch_nn_brute_queries(mvicp_ctx* c, const FrameDev& f, const double* d_q, int n, int* d_idx, double* d_d2);
int launch_nn_grid_edges(mvicp_ctx* c, double d2_bound, const SearchPlan& plan);                          // nn_grid.hip (d2_bound = the cutoff's; the search radius is search_bound())
double search_bound(const mvicp_ctx* c, double d2_bound);                               // api.cpp                              // nn_grid.hip
int launch_nn_tile_edges(mvicp_ctx* c, double d2_bound, const SearchPlan& plan);   // nn_tile.hip: the build the plan chose (tile_lb, tile_cached, cached_on_mfma)
int launch_nn_mfma_edges(mvicp_ctx* c, double d2_bound, bool with_bounds, bool with_cache, bool with_list);   // nn_mfma.hip
int build_mfma(FrameDev& f, const double* sorted_pts);                                 // nn_mfma.hip (host, called by build_grid)
int warm_nn_mfma(mvicp_ctx* c);
int warm_nn_tile(mvicp_ctx* c); int warm_nn_grid(mvicp_ctx* c);                                    // code-object load at set-up time (mvicp_set_graph)                              // nn_tile.hip
int build_wide(FrameDev& f, const double* sorted_pts);                                 // nn_tile.hip (host, called by build_grid)
int launch_nn_grid_queries(mvicp_ctx* c, const FrameDev& f, const double* d_q, int n, int* d_idx, double* d_d2);
int build_grid(mvicp_ctx* c, FrameDev& f, const double* h_xyz);
int device_bounds(hipStream_t stream, const double* d_xyz, int n, DevBounds* out);   // build.hip: the validate + bbox reduction (waits for it)
int build_grid_device(mvicp_ctx* c, FrameDev& f, const DevBounds& b, int grid_curve, double grid_target);   // build.hip: same arrays as build_grid, from f.pts
int finish_builds(mvicp_ctx* c);   // api.cpp: wait for every pending structure build of this context; first failure wins
void free_grid(GridDev& g);
void free_tie(FrameDev& f);                                                            // nn_tie.hip
// overlap.hip: census of all ordered pairs.  xf: K x K x 24 query transforms (pair i -> j at [i * K + j]); B2 = squared cutoff bound,
// scale = 2^q_exp; samples K, hits K x K, sumq K x K or null (host arrays).  Waits for the stream; history-neutral.
int overlap_census(mvicp_ctx* c, const double* xf, double B2, double scale, int max_samples, int* samples, int* hits, long long* sumq);
void free_overlap(mvicp_ctx* c);
// voxel.hip: the points of the n_sel frames sel[] (valid, distinct, uploaded), at poses (n_frames x 16) or as stored (null), reduced to one
// point per voxel; the result stays on the context (c->vox).  Returns the number of voxels or a negative status.  Waits for the stream; history-neutral.
long long voxel_reduce(mvicp_ctx* c, int n_sel, const int* sel, const double* poses, double voxel, int* has_normals);
// outlier.hip: k-distance search over frame f's hash (valid, uploaded, structures built; 1 <= k <= 32, n == 0 or n > k), the statistical
// (std_ratio >= 0) and the radius (radius > 0) rule; the result stays on the context (c->out).  Returns the number kept or a negative
// status.  Waits for the stream; history-neutral.
long long outlier_filter(mvicp_ctx* c, const FrameDev& f, int k, double std_ratio, double radius, mvicp_outlier_stats* stats);
// cluster.hip: the clusters of frame f = c->frames[frame] (valid, uploaded, structures built) for B2 = sqrt_bound(radius) and 1 <= min_pts <= 2^30;
// the result stays on the context (c->clu).  Returns the number of clusters or a negative status (coordinates whose distances can
// overflow: MVICP_ERR_ARG, no result).  Waits for the stream once; history-neutral.
long long cluster_points(mvicp_ctx* c, const FrameDev& f, int frame, double B2, int min_pts, mvicp_cluster_stats* stats);
// cluster.hip: the rows of f (the frame of the last cluster_points, unchanged since: c->clu.n == f.n >= 0) whose cluster the rule
// mvicp_cluster_keep_rule(min_size, max_clusters) keeps, compacted in ascending original index into c->clu.sel (select_rows).  Returns the rows kept or a
// negative status.  Waits for the stream once; history-neutral.
long long cluster_select(mvicp_ctx* c, const FrameDev& f, long long min_size, long long max_clusters);
// plane.hip: the dominant plane of frame f = c->frames[frame] (valid, uploaded) over H hypotheses (1 <= H <= 2^24, finite tau > 0; axis null or
// 3 finite doubles, not all zero, with cos_min in [0, 1]); the result stays on the context (c->plane).  One wait without a refit, two
// with one (the host rule mvicp_plane_from_moments stands between them); history-neutral.
int plane_segment(mvicp_ctx* c, const FrameDev& f, int frame, long long H, unsigned long long seed, double tau, const double* axis, double cos_min, int refine,
                  mvicp_plane_result* out);
// plane.hip: the rows of f (the frame of the last plane_segment, unchanged since: c->plane.n == f.n >= 0) with flag == (inliers ? 1 : 0),
// compacted in ascending original index into c->plane.sel (select_rows).  Returns the rows kept or a negative status.  Waits for the stream once.
long long plane_select(mvicp_ctx* c, const FrameDev& f, int inliers);
// boundary.hip: the boundary points of frame f = c->frames[frame] (valid, uploaded, structures built) by the normals N (n x 3 doubles on the
// device: the frame's own or the last estimate's; unread when n == 0); 3 <= max_nn <= 64, B2 = sqrt_bound(radius) when radius > 0, cos_gap in
// (-1, 1).  Runs knn_search in self mode (that search stays the context's last) and leaves the result on the context (c->bnd).  Returns the
// number of flagged points or a negative status.  Waits for the stream; otherwise history-neutral.
long long boundary_points(mvicp_ctx* c, const FrameDev& f, int frame, const double* N, int max_nn, double radius, double B2, double cos_gap);
// boundary.hip: the rows of f (the frame of the last boundary_points, unchanged since: c->bnd.n == f.n >= 0) with flag == (boundary ? 1 : 0),
// compacted in ascending original index into c->bnd.sel (select_rows).  Returns the rows kept or a negative status.  Waits for the stream once.
long long boundary_select(mvicp_ctx* c, const FrameDev& f, int boundary);
// knn.hip: the neighbourhoods of m queries (host or device memory, as `queries_on_device` says) or, queries == null, of the cloud's own
// points, in frame f (valid, uploaded, structures built); 0 <= k <= 64, k == 0 needs radius > 0; B2 = sqrt_bound(radius) when radius > 0.
// The result stays on the context (c->knn).  Returns the number of entries or a negative status.  Waits for the stream; history-neutral.
long long knn_search(mvicp_ctx* c, const FrameDev& f, const double* queries, int queries_on_device, long long m, int k, double radius, double B2);
// fpfh.hip: knn_search(c, f, null, 0, 0, max_nn, radius, B2) and the two descriptor passes over its rows, for frame f (valid, uploaded,
// with normals unless empty, structures built; 2 <= max_nn <= 64, radius > 0, B2 = sqrt_bound(radius)); the result stays on the context
// (c->fpfh), the search's in c->knn.  Returns the number of rows or a negative status.  Waits for the stream; history-neutral.
long long fpfh_compute(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2);
// match.hip: the two nearest rows of B (n x dim) for every row of A (m x dim) and the reverse; 0 <= m, n < 2^31, 1 <= dim <= 64; each
// operand in host or device memory as its `_on_device` says.  The result stays on the context (c->match).  Returns m or a negative
// status (a non-finite value: MVICP_ERR_ARG, no result).  Waits for the stream; history-neutral.
long long feature_match(mvicp_ctx* c, const double* A, int a_on_device, long long m, const double* B, int b_on_device, long long n, int dim);
// consensus.hip: H hypotheses over the n_pairs index-aligned pairs (P, Q) (host or device memory); 3 <= n_pairs < 2^31, 1 <= H <= 2^24,
// tau > 0, 0 <= edge_sim < 1.  count / flags stay on the context (c->cons), the record goes to `out`.  Returns a status (a non-finite
// coordinate: MVICP_ERR_ARG, no result).  Waits for the stream; history-neutral.
int consensus(mvicp_ctx* c, const double* P, int p_on_device, const double* Q, int q_on_device, long long n_pairs, long long H, unsigned long long seed,
              double tau, double edge_sim, mvicp_consensus_result* out);
// coarse.hip: the chain feature_match -> match_pairs -> gather -> consensus for every edge (src[e], dst[e]) over n_sets sets whose rows
// are offsets[s] .. offsets[s+1] of desc (x dim) and xyz (x 3), each in host or device memory; every argument already checked.  pairs /
// flags stay on the context (c->coarse), the records go to `results`.  Returns n_edges or a negative status (a non-finite value:
// MVICP_ERR_ARG, no result).  Waits for the stream twice, however many edges; history-neutral.
long long coarse_pairs(mvicp_ctx* c, const double* desc, int desc_on_device, const double* xyz, int xyz_on_device, const long long* offsets, int n_sets, int dim,
                       int n_edges, const int* src, const int* dst, const unsigned long long* seeds, int mutual, double ratio, long long H, double tau,
                       double edge_sim, mvicp_coarse_edge* results);
// iss.hip: the ISS keypoints of frame f (valid, uploaded, structures built) for arguments already checked; B2_* = sqrt_bound of the two
// radii, q = 20 - the binary exponent of the salient radius.  The result stays on the context (c->iss).  Returns the number of keypoints
// or a negative status (a salient row of more than 1024 points: MVICP_ERR_ARG, no result).  Waits for the stream once; history-neutral.
long long iss_keypoints(mvicp_ctx* c, const FrameDev& f, double B2_salient, double B2_nms, int q, double gamma21, double gamma32, int min_neighbors);
// normals_pca.hip: knn_search(c, f, null, 0, 0, max_nn, radius, B2) and the PCA pass over its rows, for frame f (valid, uploaded, structures
// built; 3 <= max_nn <= 64, B2 = sqrt_bound(radius) when radius > 0, viewpoint 3 finite doubles); the result stays on the context (c->nrm;
// the caller sets c->nrm.frame), the search's in c->knn.  Returns the number of rows or a negative status.  Waits for the stream; history-neutral.
long long normals_estimate(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2, const double* viewpoint);
// normals_jet.hip: the same with the jet fit of `degree` (2 or 3) behind the PCA part; the result replaces c->nrm's and carries the fitted bytes.
long long normals_fit(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2, const double* viewpoint, int degree);
// smooth.hip: the same search and fit, continued to the height a_0: the points moved onto the fitted surface along the PCA normal (max_shift
// <= 0: no limit) and the mean and Gaussian curvature.  c->nrm holds normals_fit's bytes and, in its smo part, the smoothing result.
long long smooth_points(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2, const double* viewpoint, int degree, double max_shift);
// normals_pca.hip: nrm (f.n rows, device memory) into f.nor and f.grid.snor (both allocated, f.n > 0, structures built).  Waits for the stream.
int normals_adopt(mvicp_ctx* c, FrameDev& f, const double* nrm);
// orient.hip: knn_search(c, f, null, 0, 0, k, radius, B2) and the propagation over its rows for the normals N (f.n x 3, device memory) of
// frame f (valid, uploaded, structures built; 2 <= k <= 64, mode an mvicp_orient_mode, ref 3 finite doubles); the result stays on the
// context (c->ori; the caller sets c->ori.frame), the search's in c->knn.  Returns the number of components or a negative status (a
// non-finite weight: MVICP_ERR_ARG, no result).  Waits for the stream once per round; history-neutral.
long long orient_normals(mvicp_ctx* c, const FrameDev& f, const double* N, int k, double radius, double B2, int mode, const double* ref);
// orient.hip: every stored normal of f negated in place, in original and in sorted order (f.nor and f.grid.snor non-null).  Waits for the stream.
int negate_normals(mvicp_ctx* c, FrameDev& f);
// orient.hip: per owned edge with use[e] != 0 the counts of positive / negative dots between the rotated normals of its list's pairs, at
// poses (n_frames x 16); every used edge's frames have sorted normals.  One launch, one wait; history-neutral.
int normal_agreement(mvicp_ctx* c, const double* poses, const char* use, int* pos, int* neg);
int launch_compact(mvicp_ctx* c, double d2_bound);                                    // corr.hip
int launch_gather_stream(mvicp_ctx* c);
int launch_mask_permute(mvicp_ctx* c, const FrameDev& f);                            // f.grid.omask (original order) -> f.grid.smask (sorted order)
int launch_select_median(mvicp_ctx* c, double d2_bound);   // two-pass select anchored at the acceptance bound: any key set, exact
int launch_export(mvicp_ctx* c);           // export.hip: every exportable edge's list -> reference-order triples in pinned memory (async; caller waits)
int launch_select_bracket(mvicp_ctx* c);   // one-pass select around last round's medians (d_sel_lohi); flags edges it cannot answer
int launch_linearize(mvicp_ctx* c, int plane, int robust);                            // linearize.hip
int launch_linearize_pair(mvicp_ctx* c, int plane, int robust, double* out_a, double* out_b);   // linearize.hip: d_rel -> out_a, d_rel2 -> out_b, one pass
constexpr int kMetricGicp = 3;   // the plane-to-plane objective inside the library (evaluate_blocks, check_evaluable); NOT an mvicp_metric: the metric calls refuse 3
inline bool gicp_epsilon_ok(double eps) { return eps >= 1e-6 && eps <= 1.0; }   // (false for a NaN)
int launch_linearize_gicp(mvicp_ctx* c, double eps, int robust);                      // linearize_gicp.hip: the plane-to-plane objective, the symmetric launch's tables / partials / outputs
int launch_linearize_sym(mvicp_ctx* c, int robust);                                   // linearize_sym.hip: the symmetric objective, same tables / partials / outputs as launch_linearize
int launch_normals(mvicp_ctx* c, FrameDev& f, int k, int* d_knn);                      // normals.hip
int stream_wait(mvicp_ctx* c);      // api.cpp: wait for the context's stream (spin-polls first)
void census_resolve(mvicp_ctx* c);  // api.cpp: fold the counters of the last NN launch into the profile (after a sync)

// small host->device table uploads through a persistent bump-allocated scratch buffer; the copy is a
// synchronous hipMemcpy (tables are tiny) so the pageable source may die right after the call.
// device copy of a small host table, re-uploaded only when its bytes change (job / pointer tables are the same every round)
int cached_upload(mvicp_ctx* c, const char* key, const void* src, size_t bytes, void** dptr);
void scratch_reset(mvicp_ctx* c);
int scratch_upload(mvicp_ctx* c, const void* src, size_t bytes, void** dptr);

// profiling helpers
struct ProfScope {
  mvicp_ctx* c; const char* name; hipEvent_t a = nullptr, b = nullptr; bool on;
  ProfScope(mvicp_ctx* c, const char* name, double bytes);
  ~ProfScope();
};
void prof_collect(mvicp_ctx* c);
void prof_collect_lazy(mvicp_ctx* c);   // the hot calls: only once a scope holds > 256 unresolved event pairs
// host wall-clock sections (same table, names prefixed "host."), only while profiling
struct HostScope {
  mvicp_ctx* c; const char* name; double t0; bool on;
  HostScope(mvicp_ctx* c, const char* name);
  ~HostScope();
};

}  // namespace mvicp
