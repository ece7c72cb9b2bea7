// Host-side mirror of the reference's Frame / ICP_Ceres interface on top of the C ABI (include/mvicp.h).
// Same member names, argument meaning and call order as the reference, so a driver written against
// include/frame.h + include/icp-ceres.h of adrelino/mv-lm-icp reads the same here:
//   struct Correspondance / OutgoingEdge            include/frame.h:18-29
//   class Frame                                     include/frame.h:31-102
//   ICP_Ceres::ceresOptimizer*, pointToPoint/Plane_* include/icp-ceres.h:29-42
// Differences forced by the boundary: errors are thrown as std::runtime_error carrying mvicp_last_error() (the
// reference has nothing to propagate); OutgoingEdge::P_relative (never used, frame.h:28) is dropped; draw()/GL
// members are out of scope.
//
// WHAT THE MIRROR NOTICES (the one rule; INTEGRATION.md "What the mirror notices").  The device copies, the cached search and
// the k-NN table are keyed on addresses, sizes and counters, never on the clouds' values:
//   noticed by itself   a `pts` / `nor` vector REPLACED by another one (another buffer address or another size) on a bound and on an
//                       unbound frame; `version` (recomputeNormals(), estimateNormals(), fitNormals(), orientNormals() and Session::orientFrames bump it); a Frame destroyed, or destroyed and constructed again in
//                       the same storage (~Frame() tells the session); another frames vector, other frames in it, another order, another
//                       graph; changed poses / thresh / fixed / Session::nn_method; Session::copy_back switched; any call that threw
//                       (whatever the session believed about the device copy it was uploading is forgotten before the upload starts).
//   needs invalidate()  values of `pts` / `nor` edited IN PLACE -- overwritten elements, or an assignment that reuses the vector's capacity
//                       (same address, same size): call Session::get().invalidate() before the next call.
//   the k-NN table      of getNeighbours / getNeighbourIndices is dropped by a replaced `pts` vector, by `version` and by
//                       Session::invalidate() (for in-place edits).
//   the lists           a caller that overwrites ELEMENTS of a filled correspondence list calls Session::invalidate_lists() (see `held`).
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/mvicp.h"
#include "linalg.h"

namespace mvicp {

struct Correspondance { int first; int second; double dist; };
static_assert(sizeof(Correspondance) == sizeof(mvicp_corr), "mvicp_corr is the reference's Correspondance (include/frame.h:18-22)");

struct OutgoingEdge {
  int neighbourIdx;
  float weight;  // pose distance at graph build, then 1.5 x median correspondence distance (frame.cpp:176)
  std::vector<Correspondance> correspondances;
};

class Frame {
 public:
  std::vector<Vector3d> pts;
  std::vector<Vector3d> nor;
  bool fixed = false;
  Isometry3d pose;
  Isometry3d poseGroundTruth;
  std::vector<OutgoingEdge> neighbours;
  unsigned long long version = 0;   // bumped by recomputeNormals() / estimateNormals(): the session re-uploads the cloud when it changes

  Frame() = default;
  Frame(const Frame&) = default;
  Frame& operator=(const Frame&) = default;
  ~Frame();   // tells the session: a Frame constructed later at this address is never taken for this one

  // frame.cpp:67-89 (host; tiny)
  void computePoseNeighboursKnn(std::vector<std::shared_ptr<Frame>>* frames, int i, int k);
  // frame.cpp:91-185.  The first call after any pose change runs the batched device search for ALL frames; this
  // frame's edges are then filled from it (later calls for the other frames in the same round are copies only).
  void computeClosestPointsToNeighbours(std::vector<std::shared_ptr<Frame>>* frames, float thresh);
  // frame.cpp:187-206: query in this frame's local coordinates -> squared distance, index
  double getClosestPoint(const Vector3d& query_pt, size_t& ret_index);
  // Batched form of the same call (no counterpart in the reference, whose loop asks one query at a time, frame.cpp:138): ONE device
  // launch + ONE copy for all queries instead of a launch and a synchronisation per query.  ret_index[i] / returned[i] are exactly
  // what getClosestPoint(query_pts[i], ret_index[i]) returns.  Use this in any loop over queries.
  std::vector<double> getClosestPoints(const std::vector<Vector3d>& query_pts, std::vector<size_t>& ret_index);
  // frame.cpp:244-255: PCA normals from the 10 nearest points (self included), n_z <= 0; overwrites `nor`
  void recomputeNormals();
  // Exactly specified normals (no counterpart in the reference): mvicp_estimate_normals on this cloud as it is stored -- the direction of
  // least variance of the max_nn nearest points (radius > 0: within it), turned towards `viewpoint` (this frame's local coordinates; the
  // default is the sensor origin of a view in its own frame), so that the frames of one scan agree on the side their normals point to.
  // Fills `nor` and bumps `version` as recomputeNormals() does (same place in the rule above: the session notices by itself) and returns
  // the curvatures (surface variation, one per point).  Runs in the context Session::query_context finds for this frame
  // (bin/multiview --normals_nn / --normals_radius).
  std::vector<double> estimateNormals(int max_nn, double radius = 0.0, const Vector3d& viewpoint = Vector3d());
  // Jet-fitted normals (no counterpart in the reference): mvicp_fit_normals in place of mvicp_estimate_normals -- the same normal corrected
  // by the slope of a height polynomial of `degree` 2 or 3 fitted over its tangent plane; a point whose fit is refused keeps the estimate.
  // Everything else is estimateNormals(): fills `nor`, bumps `version`, returns the curvatures (bin/multiview --normals_fit).
  std::vector<double> fitNormals(int max_nn, double radius, int degree, const Vector3d& viewpoint = Vector3d());
  // Consistent orientation without a viewpoint (no counterpart in the reference): mvicp_orient_normals on this cloud and its `nor` as they
  // are stored (source 0, MVICP_ORIENT_ANCHOR) -- the sign of point 0's normal (of every tree's lowest point) is carried along the maximum
  // spanning forest of the graph of the k nearest neighbours (radius > 0: within it) weighted by |n_i . n_j|.  Replaces `nor` and bumps
  // `version` as estimateNormals() does and returns the number of trees (1: the whole cloud agrees with itself).  Which side the cloud
  // ends on is arbitrary: Session::orientFrames makes the frames agree with each other (bin/multiview --normals_orient mst).
  int orientNormals(int k, double radius = 0.0);
  // frame.cpp:208-231: the num_results nearest points of pts[queryIdx] in this cloud — the point itself first — in the order nanoflann's
  // knnSearch returns them (ascending distance, exact ties in the tree's visiting order).  The reference runs one tree query per call; here the
  // first call for a given num_results answers ALL points of the cloud in one device launch (the k-NN kernel behind recomputeNormals, 3 <= k <= 16)
  // and keeps the index table with the frame, so a loop over queryIdx — the reference's only use, frame.cpp:249 — costs one launch.
  std::vector<Vector3d> getNeighbours(int queryIdx, size_t num_results);
  // the table behind it: pts.size() x num_results original indices, row i = the neighbours of pts[i], nearest (i itself) first
  const std::vector<int>& getNeighbourIndices(size_t num_results);
  // A coarser copy of this frame (no counterpart in the reference): one point per occupied voxel of edge `voxel` — mvicp_voxel_grid on this
  // cloud as it is stored, no pose applied: per voxel the mean of its points in ascending index and, if the frame has normals, the
  // normalised sum of theirs.  The new Frame has the reduced pts / nor and the same pose, poseGroundTruth, fixed and neighbours (index and
  // weight; the correspondence lists, whose indices refer to the full cloud, start empty).  Runs in the context Session::query_context
  // finds for this frame.  A driver registers the copies for its first rounds and hands their poses to the full frames (bin/multiview
  // --coarse_voxel / --coarse_rounds).
  std::shared_ptr<Frame> voxelDownsample(double voxel);
  // A cleaned copy of this frame (no counterpart in the reference): mvicp_outlier_filter on this cloud as it is stored -- the statistical
  // rule (mean distance to the k nearest neighbours against mean + std_ratio sigma over the cloud; std_ratio < 0: off) and the radius rule
  // (at least k neighbours within `radius`; radius <= 0: off).  The new Frame has the kept pts / nor in their original order and the same
  // pose, poseGroundTruth, fixed and neighbours (index and weight; the correspondence lists start empty).  Runs in the context
  // Session::query_context finds for this frame (bin/multiview --sor_k / --sor_ratio / --ror_radius).
  std::shared_ptr<Frame> removeOutliers(int k, double std_ratio, double radius);
  // A smoothed copy of this frame (no counterpart in the reference): mvicp_smooth_points on this cloud as it is stored -- every point moved
  // onto the height polynomial of `degree` 2 or 3 fitted through its max_nn nearest neighbours (radius > 0: within it), along its PCA normal;
  // a point whose fit is refused, or whose shift exceeds max_shift > 0, stays where it is.  The new Frame has the moved pts in their
  // original order and the same pose, poseGroundTruth, fixed and neighbours (index and weight; the correspondence lists start empty).  If
  // this frame has normals the new one has the call's fitted normals, each negated where it points against this frame's own (dot product
  // below 0), so the frame's orientation survives; otherwise it has none.  shift / moved, if given, receive the call's signed shifts and
  // moved bytes.  Runs in the context Session::query_context finds for this frame (bin/multiview --smooth_nn / --smooth_radius /
  // --smooth_degree / --smooth_iters / --smooth_max_shift).
  std::shared_ptr<Frame> smoothPoints(int max_nn, double radius, int degree, double max_shift, const Vector3d& viewpoint = Vector3d(),
                                      std::vector<double>* shift = nullptr, std::vector<unsigned char>* moved = nullptr);
  // A copy of this frame without its small clusters (no counterpart in the reference): mvicp_cluster on this cloud as it is stored -- DBSCAN
  // with the strict radius predicate, the point itself counting towards min_pts -- and mvicp_cluster_select: the points of the clusters with
  // at least min_size members, of those only the max_clusters largest (0: all of them); noise always goes.  The new Frame has the kept
  // pts / nor in their original order and the same pose, poseGroundTruth, fixed and neighbours (index and weight; the correspondence
  // lists start empty).  clusters / kept_clusters, if given, receive the number of clusters found and kept.  Runs in the context
  // Session::query_context finds for this frame (bin/multiview --cluster_radius / --cluster_min_pts / --cluster_min_size / --cluster_keep).
  std::shared_ptr<Frame> removeSmallClusters(double radius, int min_pts, long long min_size, long long max_clusters, long long* clusters = nullptr,
                                             long long* kept_clusters = nullptr);
  // A copy of this frame without its dominant plane, or of that plane alone (no counterpart in the reference): mvicp_segment_plane on this
  // cloud as it is stored -- RANSAC over `hypotheses` three-point samples of the generator seeded with `seed`, a point within tau of the plane
  // an inlier, with `axis` (3 doubles; null: any plane) only planes whose normal has |cos| >= cos_min to it, the winner refitted over its
  // inliers -- and mvicp_plane_select: the points off the refitted plane (keep_plane = false) or on it (true).  The new Frame has the kept
  // pts / nor in their original order and the same pose, poseGroundTruth, fixed and neighbours (index and weight; the correspondence
  // lists start empty).  result, if given, receives the call's record (best = -1: no plane was found and nothing is an inlier).  Runs in
  // the context Session::query_context finds for this frame (bin/multiview --plane_tau / --plane_hyp / --plane_seed / --plane_keep /
  // --plane_axis / --plane_cos).
  std::shared_ptr<Frame> removePlane(double tau, long long hypotheses = 1024, unsigned long long seed = 0, const double* axis = nullptr, double cos_min = 0.0,
                                     bool keep_plane = false, mvicp_plane_result* result = nullptr);
  // The boundary points of this frame (no counterpart in the reference): mvicp_boundary on this cloud and its `nor` as they are stored
  // (source 0) -- a point is flagged when, in its tangent plane, the directions to its max_nn nearest neighbours (radius > 0: within it)
  // leave a gap of at least acos(cos_gap) -> one byte per point, 1 = boundary.  The frame needs normals.  Runs in the context
  // Session::query_context finds for this frame (bin/multiview --reject_boundary / --boundary_nn / --boundary_radius / --boundary_cos).
  std::vector<unsigned char> boundaryPoints(int max_nn = 30, double radius = 0.0, double cos_gap = -0.5);
  // The ISS keypoints of this frame (no counterpart in the reference): mvicp_iss_keypoints on this cloud as it is stored -> the indices
  // of the keypoints, ascending.  Runs in the context Session::query_context finds for this frame (bin/multiview --feat_keypoints).
  std::vector<int> issKeypoints(double salient_radius, double non_max_radius, double gamma21 = 0.975, double gamma32 = 0.975, int min_neighbors = 5);

 private:
  // cache of getNeighbourIndices and what it was built from: k, the pts buffer and size, `version`, Session::knn_generation
  std::vector<int> knn_table_; size_t knn_k_ = 0; const void* knn_pts_ = nullptr; size_t knn_n_ = 0;
  unsigned long long knn_version_ = 0, knn_generation_ = 0;
};

// Process-wide device session behind the Frame / ICP_Ceres calls: uploads the (static) clouds once, mirrors the
// pose graph, caches the batched correspondence search of the current poses.
struct Session {
  static Session& get();
  mvicp_ctx* ctx = nullptr;
  int device = 0;
  bool copy_back = true;  // fill Frame::neighbours[].correspondances after the search (off: device-only, faster)
  int copy_threads = 8;   // host threads that slice the mapped triples into a frame's vectors (1 = the calling thread alone)
  const mvicp_corr* corr = nullptr; const long long* corr_off = nullptr;   // mvicp_map_correspondences of the current search (library-owned, pinned)
  // Copy-back bookkeeping (frame.cpp:110,156-160 clears and refills every list every round; refilling a list with the bytes it already holds
  // is skipped): per edge the library's change counter (mvicp_correspondence_epochs) of the list the Frame's vector was last filled from, and
  // the vector's buffer and length at that time — a caller that resized, cleared or re-allocated the vector gets a fresh copy.  (A caller that
  // overwrites ELEMENTS of a filled list in place and expects the next round to repair them must call Session::invalidate_lists().)
  const unsigned long long* epochs = nullptr;
  struct Held { unsigned long long epoch = 0; const void* data = nullptr; size_t n = 0; };
  std::vector<Held> held;
  unsigned long long edges_copied = 0, edges_skipped = 0;   // statistics of the copy-back (tests, bench)
  void invalidate_lists() { held.assign(held.size(), Held()); }
  int nn_method = MVICP_NN_AUTO;
  int last_nn_method = MVICP_NN_AUTO;      // of the cached search
  const void* frames_key = nullptr;
  // what the device copy was built from: per frame {Frame*, pts data, size, nor data, normals version}; any difference
  // (a re-loaded cloud, recomputeNormals(), an edited point vector) triggers a fresh upload at the next bind
  struct FrameKey { const Frame* f; const void* pts; size_t n; const void* nor; unsigned long long version;
                    bool operator==(const FrameKey& o) const { return f == o.f && pts == o.pts && n == o.n && nor == o.nor && version == o.version; } };
  std::vector<FrameKey> frame_keys;
  std::vector<int> esrc, edst;
  std::vector<double> last_poses;
  std::vector<unsigned char> last_fixed;
  float last_thresh = -1.f;
  // getClosestPoint on an unbound frame: the side context holds the cloud of side_owner as it was at side_key (frame, buffers, size, version)
  mvicp_ctx* side_ctx = nullptr; const Frame* side_owner = nullptr; unsigned long long side_version = 0;
  FrameKey side_key{nullptr, nullptr, 0, nullptr, 0};
  bool side_nor = false;                   // the side context holds the frame's normals too (voxelDownsample asks for them)
  int frame_index(const Frame* f) const;   // position of f in the bound vector, or -1
  // context + frame slot that hold `f`'s cloud for raw queries: the bound session if f is part of it, else a one-cloud side context.
  // with_normals: the slot must hold the frame's CURRENT normals as well (the bound session only if it was uploaded from them)
  mvicp_ctx* query_context(Frame* f, int* slot, bool with_normals = false);
  void invalidate();                       // forget the device copy (forces re-upload + fresh search) and every frame's k-NN table; for in-place edits of pts/nor data
  void forget(const Frame* f);             // ~Frame(): nothing the session holds is attributed to this address any more
  unsigned long long knn_generation = 1;   // bumped by invalidate(): a Frame's k-NN table of an older generation is rebuilt
  std::vector<int> counts;
  std::vector<float> weights;
  bool graph_bound = false;                                   // the context holds the graph of esrc / edst (false: clouds only)
  void upload(std::vector<std::shared_ptr<Frame>>& frames);    // the clouds alone (no graph)
  void ensure_uploaded(std::vector<std::shared_ptr<Frame>>& frames);   // upload unless the session holds exactly these clouds (a new upload drops the graph)
  // The fused model (no counterpart in the reference, whose end product is the merged cloud in its viewer): the points of ALL frames at their
  // current poses reduced to one point per voxel of edge `voxel` (mvicp_voxel_grid over every frame, in frame order).  pts / nor receive the
  // rows in output order; nor stays empty when a non-empty frame has no normals.  Returns the number of voxels.
  long long fusedModel(std::vector<std::shared_ptr<Frame>>& frames, double voxel, std::vector<Vector3d>& pts, std::vector<Vector3d>& nor);
  void bind(std::vector<std::shared_ptr<Frame>>& frames);      // upload + graph (idempotent)
  // Pose graph from the overlap census (mvicp_overlap + mvicp_graph_from_overlap) in place of the computePoseNeighboursKnn loop
  // (main_multiview.cpp:104-117): fills EVERY Frame::neighbours with the frame's knn best-overlapping frames at the current poses
  // (weight = 1 - fraction of the frame's samples with a counterpart within thresh) and returns the number of connected components.
  // More than one component is reported, not repaired: frames cut off from frame 0 make the solve singular.
  int computeOverlapNeighbours(std::vector<std::shared_ptr<Frame>>& frames, int knn, float thresh, int max_samples = 4096, double min_fraction = 0.0);
  // Initial poses from the clouds alone (no counterpart in the reference, which starts from pose files): FPFH descriptors of every frame
  // (mvicp_fpfh; of its voxelDownsample(voxel) copy when voxel > 0), ONE mvicp_coarse_pairs over all edges i < j with seeds[e] = seed + e,
  // mutual matches, no ratio test; with `refine` mvicp_closedform_point_to_point over each edge's inliers (when there are at least 3);
  // mvicp_poses_from_pairs over the inlier counts from root 0 at frames[0]->pose.  Writes frames[i]->pose for i >= 1 and returns the
  // number of components (more than one is reported, not repaired: a frame no usable edge reaches stands at the identity).  `edges`
  // receives one record per edge.  The frames need normals.
  // keypoints = 1 or 2: the descriptors are still computed on the whole cloud that carries the features, mvicp_iss_keypoints selects rows
  // of every frame (`keypoints` receives how many of how many), and only the selected rows are matched -- 1: the keypoints of both frames of an
  // edge; 2: the keypoints of the source against every point of the destination (2 K sets: the keypoints, then the clouds; edge (i, j)
  // becomes (i, K + j)).  The refinement uses the rows that were matched.
  struct FeatureInit {
    double voxel = 0.0, radius = 0.0, tau = 0.0, edge_sim = 0.9;
    int max_nn = 64, min_count = 3;
    long long hypotheses = 10000;
    unsigned long long seed = 0;
    bool refine = true;
    int keypoints = 0;   // 0: none, 1: both sides, 2: the source side only
    double salient_radius = 0.0, nms_radius = 0.0, gamma21 = 0.975, gamma32 = 0.975;
    int min_neighbors = 5;
  };
  struct FeatureEdge { int src, dst, pairs, accepted, inliers; };
  struct FeatureKeypoints { int keypoints, points; };   // of the cloud that carries the frame's features
  int initFromFeatures(std::vector<std::shared_ptr<Frame>>& frames, const FeatureInit& opts, std::vector<FeatureEdge>* edges = nullptr,
                       std::vector<FeatureKeypoints>* keypoints = nullptr);
  void correspond(std::vector<std::shared_ptr<Frame>>& frames, float thresh);
  // The step between the clouds of a consistent orientation (every frame consistent in itself, e.g. by Frame::orientNormals, and the graph
  // built): one search at the current poses, mvicp_normal_agreement over its lists, mvicp_signs_from_agreement over the graph's edges (an
  // edge is usable with at least min_count pairs); the normals of every frame the rule flips are negated (a replaced `nor` vector and a
  // bumped `version`: the next bind uploads them).  `flipped` receives one flag per frame.  Returns the number of components of the sign
  // graph (more than one is reported, not repaired).
  int orientFrames(std::vector<std::shared_ptr<Frame>>& frames, float thresh, int min_count = 0, std::vector<unsigned char>* flipped = nullptr);
  // Rejects the pairs that end on a flagged point of their target (Rusinkiewicz & Levoy 2001, section 3.4: for views that overlap only in
  // part), AFTER every frame's computeClosestPointsToNeighbours of a round and BEFORE its solve, with copy_back on: masks[j] is one byte per
  // point of frames[j] (Frame::boundaryPoints; an empty mask flags nothing).  Entries whose `second` is flagged are erased from
  // frames[i]->neighbours[k].correspondances, in their order, and every list that lost an entry is installed with
  // mvicp_set_correspondences at the searched weight, so that the solve sees what the Frame holds.  The installed lists are explicit (their
  // distances read 0 in the library) and have a new epoch; the session forgets the round's search and what it held of the changed lists,
  // so the next computeClosestPointsToNeighbours searches again -- like a first search, the temporal cache is gone -- and refills.
  // Returns the pairs dropped per edge, in edge order.
  std::vector<long long> rejectBoundary(std::vector<std::shared_ptr<Frame>>& frames, const std::vector<std::vector<unsigned char>>& masks);
  // The same rejection INSIDE the search (mvicp_set_reject_mask), set ONCE for a frames vector and called in no round: masks[j] is one byte
  // per point of frames[j] (an empty mask, or roles 0, clears that frame's), applied in `roles` (MVICP_REJECT_AS_TARGET / _AS_SOURCE, or-ed).
  // Every later computeClosestPointsToNeighbours over these frames drops the pairs on flagged points on the device: the lists stay searched
  // lists (temporal cache, in-place upkeep, queued evaluations), copy_back is not needed, and with it on the Frame's vectors receive the
  // filtered lists through the ordinary copy-back.  The edge's weight is the median over the KEPT pairs (rejectBoundary keeps the
  // unfiltered list's).  The session keeps the masks and installs them again whenever it uploads this frames vector; masks set for
  // another vector (a coarse level) are replaced.  The cached round, if any, is forgotten: the next search runs.
  void setRejectMasks(std::vector<std::shared_ptr<Frame>>& frames, const std::vector<std::vector<unsigned char>>& masks, int roles = MVICP_REJECT_AS_TARGET);
  std::vector<std::vector<unsigned char>> reject_masks; int reject_roles = 0; const void* reject_key = nullptr;   // what setRejectMasks was given last
  void install_reject_masks(const std::vector<std::shared_ptr<Frame>>& frames);   // the kept masks into the context that holds `frames`
  void optimize(std::vector<std::shared_ptr<Frame>>& frames, int param, bool pointToPlane, bool robust, mvicp_summary* sm = nullptr);
  // the same with the objective named (MVICP_METRIC_SYMMETRIC needs normals on every frame, oriented consistently)
  void optimize(std::vector<std::shared_ptr<Frame>>& frames, int param, mvicp_metric metric, bool robust, mvicp_summary* sm = nullptr);
  // the plane-to-plane (Generalized-ICP) objective at the given epsilon (mvicp_optimize_gicp): needs normals on every frame, in any orientation
  void optimizeGicp(std::vector<std::shared_ptr<Frame>>& frames, int param, double epsilon, bool robust, mvicp_summary* sm = nullptr);
  void reset();
};

}  // namespace mvicp

namespace ICP_Ceres {
using mvicp::Frame;
using mvicp::Isometry3d;
using mvicp::Vector3d;
// multiview (icp-ceres.h:40-42)
void ceresOptimizer(std::vector<std::shared_ptr<Frame>>& frames, bool pointToPlane, bool robust);
void ceresOptimizer_ceresAngleAxis(std::vector<std::shared_ptr<Frame>>& frames, bool pointToPlane, bool robust);
void ceresOptimizer_sophusSE3(std::vector<std::shared_ptr<Frame>>& frames, bool pointToPlane, bool robust, bool automaticDiffLocalParam = true);
// pairwise (icp-ceres.h:30-36): returns the src -> dst transform, starting from identity
Isometry3d pointToPoint_EigenQuaternion(std::vector<Vector3d>& src, std::vector<Vector3d>& dst);
Isometry3d pointToPoint_CeresAngleAxis(std::vector<Vector3d>& src, std::vector<Vector3d>& dst);
Isometry3d pointToPoint_SophusSE3(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, bool automaticDiffLocalParam = true);
Isometry3d pointToPlane_EigenQuaternion(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, std::vector<Vector3d>& nor);
Isometry3d pointToPlane_CeresAngleAxis(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, std::vector<Vector3d>& nor);
Isometry3d pointToPlane_SophusSE3(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, std::vector<Vector3d>& nor, bool automaticDiffLocalParam = true);
}  // namespace ICP_Ceres

namespace ICP_Closedform {
using mvicp::Isometry3d;
using mvicp::Vector3d;
// include/icp-closedform.h:10-11 (host only): comparison baselines of main_pairwise.cpp:74-76,93-95
Isometry3d pointToPlane(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, std::vector<Vector3d>& nor);
Isometry3d pointToPoint(std::vector<Vector3d>& src, std::vector<Vector3d>& dst);
}  // namespace ICP_Closedform
