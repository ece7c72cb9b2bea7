// The Frame / Session / ICP_Ceres mirror (mv-lm-icp_amd/host/frame.h) behind a plain C boundary, so that the Python suite can drive
// it in any order (tests/framelib.py, tests/test_gpu_frame_mirror.py).  Built as mv-lm-icp_amd/bin/frame_harness.so from this file and
// host/frame.cpp, linked against libmvicp_hip.so.  Every call returns 0, or -1 after an exception whose text fh_last_error() holds.
//
// Frames live in storage the harness owns ("slots"): a slot's Frame can be destroyed and constructed again AT THE SAME ADDRESS (explicit
// destructor + placement new), and the vectors of frames hold shared_ptrs with a no-op deleter.  There are two vector objects (v = 0, 1),
// so that the same frames can be handed to the mirror through another vector.  A `pts` / `nor` vector is replaced by one that is
// allocated WHILE the old one still exists (so its buffer address differs by construction), or overwritten element by element in place.
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../mv-lm-icp_amd/host/frame.h"

using namespace mvicp;

namespace {

struct Slot {
  alignas(Frame) unsigned char raw[sizeof(Frame)];
  bool alive = false;
  Frame* frame() { return reinterpret_cast<Frame*>(raw); }
};

std::vector<std::unique_ptr<Slot>> g_slots;
typedef std::vector<std::shared_ptr<Frame>> FrameVec;
FrameVec* g_vec[2] = {nullptr, nullptr};
std::string g_error;
// the last result of voxelDownsample / removeOutliers / fusedModel (points, normals) and of issKeypoints (indices)
std::vector<Vector3d> g_res_pts, g_res_nor;
std::vector<int> g_res_idx;
std::vector<Vector3d> g_stash;   // a cloud vector kept aside: fh_stash_swap_pts exchanges it with a frame's `pts` (buffers and all)

struct Fail : std::exception {
  std::string msg;
  explicit Fail(const std::string& m) : msg("frame_harness: " + m) {}
  const char* what() const noexcept override { return msg.c_str(); }
};

Frame& slot(int s) {
  if (s < 0 || (size_t)s >= g_slots.size()) throw Fail("no such slot");
  if (!g_slots[s]->alive) throw Fail("the slot's frame is destroyed");
  return *g_slots[s]->frame();
}

FrameVec& vec(int v) {
  if (v < 0 || v > 1 || !g_vec[v]) throw Fail("no such vector");
  return *g_vec[v];
}

void no_delete(Frame*) {}

// mode 0: a vector allocated while the old one still exists, then swapped in; mode 1: the elements overwritten in place (same size only)
void assign_cloud(std::vector<Vector3d>& dst, const double* xyz, int n, int mode) {
  if (n < 0 || (n > 0 && !xyz)) throw Fail("bad cloud");
  if (mode == 1) {
    if ((size_t)n != dst.size()) throw Fail("an in-place overwrite keeps the size");
    if (n) std::memcpy(dst[0].data(), xyz, 24 * (size_t)n);
    return;
  }
  std::vector<Vector3d> fresh((size_t)n);
  if (n) std::memcpy(fresh[0].data(), xyz, 24 * (size_t)n);
  if (n && !dst.empty() && (const void*)fresh[0].data() == (const void*)dst[0].data()) throw Fail("the fresh vector shares the old buffer");
  dst.swap(fresh);   // (the old buffer is freed when `fresh` ends, after the new one was allocated)
}

long long fetch_cloud(const std::vector<Vector3d>& src, double* out, long long cap) {
  if (out) {
    if (cap < (long long)src.size()) throw Fail("capacity too small");
    if (!src.empty()) std::memcpy(out, src[0].data(), 24 * src.size());
  }
  return (long long)src.size();
}

void keep_result(const Frame& f) { g_res_pts = f.pts; g_res_nor = f.nor; }

}  // namespace

#define FH_TRY try {
#define FH_END \
  return 0;    \
  }            \
  catch (const std::exception& ex) { g_error = ex.what(); return -1; } \
  catch (...) { g_error = "frame_harness: unknown exception"; return -1; }

extern "C" {

const char* fh_last_error(void) { return g_error.c_str(); }

// Session::reset(), every frame destroyed, both vectors gone, the options at their defaults
int fh_reset_all(void) {
  FH_TRY
  Session& S = Session::get();
  S.reset();
  for (int v = 0; v < 2; ++v) { delete g_vec[v]; g_vec[v] = nullptr; }
  for (auto& s : g_slots) if (s->alive) { s->frame()->~Frame(); s->alive = false; }
  g_slots.clear();
  S.copy_back = true; S.copy_threads = 8; S.nn_method = MVICP_NN_AUTO;
  g_res_pts.clear(); g_res_nor.clear(); g_res_idx.clear();
  std::vector<Vector3d>().swap(g_stash);
  FH_END
}

// ---- frames in harness-owned storage
int fh_slot_create(int* out) {
  FH_TRY
  g_slots.emplace_back(new Slot());
  new (g_slots.back()->raw) Frame();
  g_slots.back()->alive = true;
  *out = (int)g_slots.size() - 1;
  FH_END
}

int fh_slot_destroy(int s) {
  FH_TRY
  slot(s).~Frame();
  g_slots[s]->alive = false;
  FH_END
}

// a new Frame (version 0, no cloud) at the address of the destroyed one
int fh_slot_recreate(int s) {
  FH_TRY
  if (s < 0 || (size_t)s >= g_slots.size()) throw Fail("no such slot");
  if (g_slots[s]->alive) throw Fail("destroy the slot's frame first");
  new (g_slots[s]->raw) Frame();
  g_slots[s]->alive = true;
  FH_END
}

int fh_slot_address(int s, unsigned long long* out) {
  FH_TRY
  if (s < 0 || (size_t)s >= g_slots.size()) throw Fail("no such slot");
  *out = (unsigned long long)(size_t)g_slots[s]->raw;
  FH_END
}

// vector v <- the frames of these slots in this order (the vector OBJECT stays the same one once it exists)
int fh_vec_set(int v, const int* slots, int n) {
  FH_TRY
  if (v < 0 || v > 1) throw Fail("no such vector");
  if (!g_vec[v]) g_vec[v] = new FrameVec();
  FrameVec next;
  for (int i = 0; i < n; ++i) next.push_back(std::shared_ptr<Frame>(&slot(slots[i]), no_delete));
  g_vec[v]->assign(next.begin(), next.end());
  FH_END
}

int fh_vec_destroy(int v) {
  FH_TRY
  if (v < 0 || v > 1) throw Fail("no such vector");
  delete g_vec[v];
  g_vec[v] = nullptr;
  FH_END
}

// ---- a frame's members
int fh_set_pts(int s, const double* xyz, int n, int mode) { FH_TRY assign_cloud(slot(s).pts, xyz, n, mode); FH_END }
int fh_set_nor(int s, const double* xyz, int n, int mode) { FH_TRY assign_cloud(slot(s).nor, xyz, n, mode); FH_END }
int fh_get_pts(int s, double* out, long long cap, long long* n) { FH_TRY *n = fetch_cloud(slot(s).pts, out, cap); FH_END }
int fh_get_nor(int s, double* out, long long cap, long long* n) { FH_TRY *n = fetch_cloud(slot(s).nor, out, cap); FH_END }
int fh_stash_set(const double* xyz, int n) { FH_TRY assign_cloud(g_stash, xyz, n, 0); FH_END }
int fh_stash_swap_pts(int s) { FH_TRY slot(s).pts.swap(g_stash); FH_END }
int fh_set_pose(int s, const double* m16) { FH_TRY std::memcpy(slot(s).pose.data(), m16, 128); FH_END }
int fh_get_pose(int s, double* m16) { FH_TRY std::memcpy(m16, slot(s).pose.data(), 128); FH_END }
int fh_set_fixed(int s, int fixed) { FH_TRY slot(s).fixed = fixed != 0; FH_END }
int fh_get_fixed(int s, int* fixed) { FH_TRY *fixed = slot(s).fixed ? 1 : 0; FH_END }
int fh_get_version(int s, unsigned long long* version) { FH_TRY *version = slot(s).version; FH_END }

int fh_set_neighbours(int s, const int* idx, const float* weight, int n) {
  FH_TRY
  Frame& f = slot(s);
  f.neighbours.clear();
  for (int j = 0; j < n; ++j) f.neighbours.push_back(OutgoingEdge{idx[j], weight ? weight[j] : 0.f, {}});
  FH_END
}

int fh_num_neighbours(int s, int* n) { FH_TRY *n = (int)slot(s).neighbours.size(); FH_END }

// edge j of the frame: the neighbour, the weight, the list's length and, with `out`, its triples
int fh_get_edge(int s, int j, int* neighbour, float* weight, long long* count, void* out, long long cap) {
  FH_TRY
  Frame& f = slot(s);
  if (j < 0 || (size_t)j >= f.neighbours.size()) throw Fail("no such edge");
  const OutgoingEdge& e = f.neighbours[j];
  *neighbour = e.neighbourIdx; *weight = e.weight; *count = (long long)e.correspondances.size();
  if (out) {
    if (cap < *count) throw Fail("capacity too small");
    if (*count) std::memcpy(out, e.correspondances.data(), sizeof(Correspondance) * e.correspondances.size());
  }
  FH_END
}

// ---- the session's options and statistics
int fh_set_option(int which, int value) {
  FH_TRY
  Session& S = Session::get();
  if (which == 0) S.copy_back = value != 0;
  else if (which == 1) S.copy_threads = value;
  else if (which == 2) S.nn_method = value;
  else throw Fail("no such option");
  FH_END
}

int fh_counters(unsigned long long* copied, unsigned long long* skipped) {
  FH_TRY
  *copied = Session::get().edges_copied; *skipped = Session::get().edges_skipped;
  FH_END
}

int fh_invalidate(void) { FH_TRY Session::get().invalidate(); FH_END }
int fh_invalidate_lists(void) { FH_TRY Session::get().invalidate_lists(); FH_END }
int fh_session_reset(void) { FH_TRY Session::get().reset(); FH_END }

// ---- the reference's calls
int fh_pose_knn(int v, int i, int k) {
  FH_TRY
  FrameVec& fr = vec(v);
  if (i < 0 || (size_t)i >= fr.size()) throw Fail("no such frame");
  fr[i]->computePoseNeighboursKnn(&fr, i, k);
  FH_END
}

int fh_closest_to_neighbours(int v, int i, float thresh) {
  FH_TRY
  FrameVec& fr = vec(v);
  if (i < 0 || (size_t)i >= fr.size()) throw Fail("no such frame");
  fr[i]->computeClosestPointsToNeighbours(&fr, thresh);
  FH_END
}

// which = 0 ceresOptimizer, 1 ceresOptimizer_ceresAngleAxis, 2 ceresOptimizer_sophusSE3
int fh_ceres(int v, int which, int point_to_plane, int robust) {
  FH_TRY
  FrameVec& fr = vec(v);
  if (which == 0) ICP_Ceres::ceresOptimizer(fr, point_to_plane != 0, robust != 0);
  else if (which == 1) ICP_Ceres::ceresOptimizer_ceresAngleAxis(fr, point_to_plane != 0, robust != 0);
  else if (which == 2) ICP_Ceres::ceresOptimizer_sophusSE3(fr, point_to_plane != 0, robust != 0);
  else throw Fail("no such optimizer");
  FH_END
}

int fh_optimize(int v, int param, int metric, int robust, mvicp_summary* summary) {
  FH_TRY
  Session::get().optimize(vec(v), param, (mvicp_metric)metric, robust != 0, summary);
  FH_END
}

int fh_get_closest_point(int s, const double* q, long long* index, double* d2) {
  FH_TRY
  size_t idx = 0;
  *d2 = slot(s).getClosestPoint(Vector3d(q[0], q[1], q[2]), idx);
  *index = (long long)idx;
  FH_END
}

int fh_get_closest_points(int s, const double* q, int n, long long* index, double* d2) {
  FH_TRY
  std::vector<Vector3d> qs((size_t)n);
  if (n) std::memcpy(qs[0].data(), q, 24 * (size_t)n);
  std::vector<size_t> idx;
  const std::vector<double> d = slot(s).getClosestPoints(qs, idx);
  if (idx.size() != (size_t)n || d.size() != (size_t)n) throw Fail("getClosestPoints returned another number of answers");
  for (int i = 0; i < n; ++i) { index[i] = (long long)idx[i]; d2[i] = d[i]; }
  FH_END
}

// out: k x 3 doubles
int fh_get_neighbours(int s, int query, int k, double* out) {
  FH_TRY
  const std::vector<Vector3d> nb = slot(s).getNeighbours(query, (size_t)k);
  if (nb.size() != (size_t)k) throw Fail("getNeighbours returned another number of points");
  if (k) std::memcpy(out, nb[0].data(), 24 * nb.size());
  FH_END
}

int fh_get_neighbour_indices(int s, int k, int* out, long long cap) {
  FH_TRY
  const std::vector<int>& t = slot(s).getNeighbourIndices((size_t)k);
  if (cap < (long long)t.size()) throw Fail("capacity too small");
  if (!t.empty()) std::memcpy(out, t.data(), sizeof(int) * t.size());
  FH_END
}

int fh_recompute_normals(int s) { FH_TRY slot(s).recomputeNormals(); FH_END }

// ---- stages whose result is a cloud or an index list: kept here, read with fh_result_*
int fh_voxel_downsample(int s, double voxel, long long* n_pts, long long* n_nor) {
  FH_TRY
  const std::shared_ptr<Frame> r = slot(s).voxelDownsample(voxel);
  keep_result(*r);
  *n_pts = (long long)g_res_pts.size(); *n_nor = (long long)g_res_nor.size();
  FH_END
}

int fh_remove_outliers(int s, int k, double std_ratio, double radius, long long* n_pts, long long* n_nor) {
  FH_TRY
  const std::shared_ptr<Frame> r = slot(s).removeOutliers(k, std_ratio, radius);
  keep_result(*r);
  *n_pts = (long long)g_res_pts.size(); *n_nor = (long long)g_res_nor.size();
  FH_END
}

int fh_iss_keypoints(int s, double salient_radius, double non_max_radius, double gamma21, double gamma32, int min_neighbors, long long* n_idx) {
  FH_TRY
  g_res_idx = slot(s).issKeypoints(salient_radius, non_max_radius, gamma21, gamma32, min_neighbors);
  *n_idx = (long long)g_res_idx.size();
  FH_END
}

int fh_fused_model(int v, double voxel, long long* n_pts, long long* n_nor) {
  FH_TRY
  const long long m = Session::get().fusedModel(vec(v), voxel, g_res_pts, g_res_nor);
  if (m != (long long)g_res_pts.size()) throw Fail("fusedModel returned another number of voxels than points");
  *n_pts = (long long)g_res_pts.size(); *n_nor = (long long)g_res_nor.size();
  FH_END
}

int fh_result_cloud(double* pts, double* nor) {
  FH_TRY
  if (pts && !g_res_pts.empty()) std::memcpy(pts, g_res_pts[0].data(), 24 * g_res_pts.size());
  if (nor && !g_res_nor.empty()) std::memcpy(nor, g_res_nor[0].data(), 24 * g_res_nor.size());
  FH_END
}

int fh_result_indices(int* idx) {
  FH_TRY
  if (idx && !g_res_idx.empty()) std::memcpy(idx, g_res_idx.data(), sizeof(int) * g_res_idx.size());
  FH_END
}

int fh_overlap_neighbours(int v, int knn, float thresh, int max_samples, double min_fraction, int* components) {
  FH_TRY
  *components = Session::get().computeOverlapNeighbours(vec(v), knn, thresh, max_samples, min_fraction);
  FH_END
}

// opts: voxel, radius, tau, edge_sim, max_nn, min_count, hypotheses, seed, refine, keypoints, salient_radius, nms_radius, gamma21, gamma32,
// min_neighbors (15 doubles, Session::FeatureInit in declaration order)
int fh_init_from_features(int v, const double* opts, int* components, int* n_edges) {
  FH_TRY
  Session::FeatureInit o;
  o.voxel = opts[0]; o.radius = opts[1]; o.tau = opts[2]; o.edge_sim = opts[3];
  o.max_nn = (int)opts[4]; o.min_count = (int)opts[5]; o.hypotheses = (long long)opts[6]; o.seed = (unsigned long long)opts[7];
  o.refine = opts[8] != 0.0; o.keypoints = (int)opts[9];
  o.salient_radius = opts[10]; o.nms_radius = opts[11]; o.gamma21 = opts[12]; o.gamma32 = opts[13]; o.min_neighbors = (int)opts[14];
  std::vector<Session::FeatureEdge> edges;
  *components = Session::get().initFromFeatures(vec(v), o, &edges, nullptr);
  *n_edges = (int)edges.size();
  FH_END
}

}  // extern "C"
