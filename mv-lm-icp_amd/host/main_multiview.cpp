// Headless counterpart of the reference's src/main_multiview.cpp (same flags, same loop, no viewer):
//   loadFrames (:53-100) -> frames[0]->fixed = true (:141) -> computePoseNeighbours (:104-117, once) ->
//   20 x { computeClosestPoints (:119-127) ; ceresOptimizer* (:158-161) }
// Extra flags: --rounds (20), --out DIR (write final poses as pose_<i>.txt, 4x4 row-major), --device, --copyback (default on: fill
// Frame::neighbours[].correspondances every round — one device un-sort + one pinned copy for all edges, sliced by --copy_threads (8) host threads),
// --drop_phantom_row (load exactly the files' rows; default: the reference's loadXYZ, which appends a duplicate of the last row),
// --noise_stream libstdc++|libc++ (std::normal_distribution's variate order for addNoise; default = this build's libstdc++), --quiet, --dump_corr DIR (after the LAST round's search
// write every Frame::neighbours[j] as corr_<src>_<j>.txt: a header line `dst weight count`, then `first second dist` rows),
// --check_nn N (re-ask Frame::getClosestPoint for the first N correspondences of every edge and report disagreements),
// --trace FILE (every round: one line `C round src j dst count weight-bits` per edge after the search and one line `P round frame m00 .. m33`
// (4x4 row-major, 17 digits) per frame after the solve: the run's whole trajectory, for parity tests against a recorded one),
// --freeze_from R (rounds >= R search but do not solve: the poses stay bit-identical), --perturb_frame K --perturb_round R (before round R's search
// frame K's translation moves by 1e-4 m), --copy_stats (one line `copyback: round r copied X skipped Y` per round): the copy-back bookkeeping of
// host/frame.h under test; --dump_corr also writes the poses of the last search (search_pose_<i>.txt); --dump_knn FILE [--knn_k 10]: Frame::getNeighbours
// (frame.cpp:208-231) of EVERY point of frame 0, asked one by one like frame.cpp:249, as raw doubles (n x k x 3), then exit.
// --graph pose|overlap (default pose = computePoseNeighboursKnn, :104-117): overlap builds the pose graph from the overlap census of the
// initial poses instead (Session::computeOverlapNeighbours: every frame keeps the --knn frames it shares most surface with) and prints one
// more line, `overlap graph: C component(s)`; --overlap_cutoff X (default --cutoff), --overlap_samples N (4096; 0 = every point),
// --overlap_min F (0: smallest share of a frame's samples that makes a candidate).
// --coarse_voxel H --coarse_rounds R (default R = 0 = off): coarse to fine — the first R of the --rounds rounds run on Frame::voxelDownsample(H)
// copies of the frames (one point per voxel of edge H; taken after recomputeNormals, normals are not recomputed on the coarse level), the
// graph is built once from the full-resolution frames, the poses after round R go to the full-resolution frames, which run the remaining
// rounds (the session re-binds by itself when the frame vector changes); --trace lines keep their format.
// --fused_out FILE --fused_voxel H: after the last round the fused model of ALL frames at the final poses (Session::fusedModel: one point per
// voxel of edge H) is written to FILE in the `.xyz` row format, `x y z nx ny nz` with 17 significant digits (`x y z` when a frame has no
// normals): exactly one row per voxel, in output order, no count line.
// --sor_k K --sor_ratio A --ror_radius R (default K = 0 = off): every frame is cleaned after loading, before recomputeNormals and before any
// coarse level, by Frame::removeOutliers(K, A, R): the statistical rule over the K nearest neighbours (A < 0, the default without --sor_ratio
// when only a radius is given: off; --sor_ratio alone defaults to 2) and / or the radius rule (at least K neighbours within R; R <= 0: off).
// One line per frame, `outlier filter: frame i kept a of b` (printed with --quiet too).
// --cluster_radius R [--cluster_min_pts M] [--cluster_min_size S] [--cluster_keep N] (default R = 0 = off; M = 4, S = 0, N = 0 = all): with R > 0
// every frame loses its small clusters after the outlier filter and before the normals step and any coarse level, by
// Frame::removeSmallClusters(R, M, S, N): the clusters of mvicp_cluster (DBSCAN: a core point has M points, itself included, within R) with at
// least S members, of those the N largest; noise always goes.  What the outlier rules keep -- a compact clump of stray points -- goes here.
// One line per frame, `cluster filter: frame i kept a of b, c of d clusters` (printed with --quiet too).
// --plane_tau T [--plane_hyp H] [--plane_seed S] [--plane_keep rest|plane] [--plane_axis=x,y,z --plane_cos C] (default T = 0 = off; H = 1024,
// S = 0, rest, no axis, C = 0): with T > 0 every frame loses its dominant plane (or, with --plane_keep plane, everything else) after the outlier
// filter and before the cluster filter, by Frame::removePlane(T, H, S, axis, C, keep): mvicp_segment_plane's RANSAC plane, refitted over its
// inliers; with an axis only planes whose normal has |cos| >= C to it.  The table, floor or turntable that joins the objects standing on it into
// one cluster goes here.  One line per frame, `plane filter: frame i kept a of b, c inliers, plane nx ny nz d` (%.17g; printed with --quiet too).
// --init features: the initial poses of frames 1 .. K-1 come from the clouds alone (Session::initFromFeatures, after loadFrames and before the
// graph is built; frame 0 keeps its loaded pose): FPFH descriptors, one batched matching + consensus over all frame pairs, a spanning tree
// over the inlier counts.  --feat_voxel H (0 = the full clouds; otherwise Frame::voxelDownsample(H) copies carry the features),
// --feat_radius (the FPFH radius; default 5 H), --feat_max_nn (64), --feat_tau (the inlier distance; default 1.5 H), --feat_hyp (10000),
// --feat_edge_sim (0.9), --feat_min_count (3: the fewest inliers that make an edge usable), --feat_seed (0), --feat_refine (default on:
// each usable pose is refined over its inliers in closed form).  One line per edge, `feature init: edge i j pairs P accepted A inliers C`,
// and one line `feature init: N component(s)` (printed with --quiet too).
// --feat_keypoints none|iss|iss_src (default none): the descriptors are still computed on every point, but only ISS keypoints are matched
// (iss: on both sides of every edge; iss_src: the keypoints of the source against every point of the destination).  --feat_salient_radius
// (default --feat_radius), --feat_nms_radius (default 0.3 x salient), --feat_gamma21, --feat_gamma32 (0.975), --feat_min_neighbors (5).
// One more line per frame, before the edge lines: `feature init: frame i keypoints k of n`.
// --symmetric (default off): the solves minimise the symmetric point-to-plane objective (MVICP_METRIC_SYMMETRIC, include/mvicp.h) instead of
// the one --pointToPlane selects, in the parameterisation the other flags select.  It needs normals on every frame (the clouds' own or
// --recomputeNormals), oriented consistently between the frames (--normals_nn below makes such normals).
// --gicp [--gicp_epsilon E] (default off; E = 1e-3, within [1e-6, 1]): the solves minimise the plane-to-plane objective of Generalized-ICP
// (mvicp_optimize_gicp, include/mvicp.h) with the covariances I - (1 - E) n n^T.  It needs normals on every frame, in any orientation.
// Together with --symmetric it is refused.
// --normals_nn K [--normals_radius R] (default K = 0 = off): with K > 0 the normals of every frame come from Frame::estimateNormals(K, R) in
// place of the recomputeNormals step (after the outlier filter, before any coarse level): the exactly specified normals of
// mvicp_estimate_normals over the K nearest points (3 <= K <= 64; R > 0: within R), turned towards the view's own origin -- the sensor of a
// range image in its own frame -- so that all frames agree on the side their normals point to, which --symmetric and --init features need.
// --normals_fit D (default 0 = off; D = 2 or 3, needs --normals_nn K): Frame::fitNormals(K, R, D) in place of Frame::estimateNormals(K, R) -- the
// same normals corrected by the slope of a height polynomial of degree D fitted over the tangent plane (mvicp_fit_normals).  Composes with
// --normals_orient and --symmetric.
// --smooth_nn K [--smooth_radius R] [--smooth_degree D] [--smooth_iters I] [--smooth_max_shift S] (default K = 0 = off; R = 0 = no radius, D = 2,
// I = 1, S = 0 = no limit): with K > 0 every frame is smoothed after the cluster filter and before the normals step, I times over, by
// Frame::smoothPoints(K, R, D, S): mvicp_smooth_points moves every point onto the height polynomial of degree D fitted through its K nearest
// neighbours, along its PCA normal (jet smoothing), unless that moves it by more than S.  Sensor noise along the normal, which every later
// stage otherwise receives unchanged, goes here.  A frame with normals keeps their orientation.  One line per frame, `smooth: frame i moved
// a of b, largest |shift| s` (the last pass; %.17g; printed with --quiet too).  D outside {2, 3}, I < 1 and a --smooth_* flag without
// --smooth_nn are refused.
// --normals_orient mst [--orient_nn K] (default off; K = 10): consistent orientation WITHOUT a viewpoint, for clouds whose frame origin is no
// sensor.  Per frame, after the normals step: Frame::orientNormals(K) (mvicp_orient_normals: the signs are carried along the maximum spanning
// forest of the K-nearest-neighbour graph weighted by |n_i . n_j|); then once across the frames, at the start poses, after the graph is built
// and before round 0: Session::orientFrames (one search, the agreement of the normals over its lists, a spanning forest over the frames;
// the frames it flips are negated).  One line per frame, `normal orientation: frame i trees t`, and one line
// `normal orientation: C component(s), flipped f0 f1 ..` (printed with --quiet too).
// --reject_boundary [--boundary_nn K] [--boundary_radius R] [--boundary_cos=C] (default off; K = 30, R = 0 = no radius, C = -0.5; a negative C needs the = form): pairs whose
// target is a boundary point of its cloud are dropped every round between the search and the solve (Rusinkiewicz & Levoy 2001, section 3.4:
// for views that overlap only in part, where source points outside the overlap find their nearest neighbour on the rim of the target).  The
// masks are Frame::boundaryPoints(K, R, C) -- mvicp_boundary on the frame's stored normals: a gap of at least acos(C) between the directions
// to the K nearest neighbours -- computed once per frame after the pre-processing flags (and once per coarse copy); Session::rejectBoundary
// applies them.  One line per frame, `boundary: frame i flagged a of b`, and one per round, `boundary: round r dropped n pairs` (printed with
// --quiet too).  Refused when a frame has no normals after pre-processing, when C is outside (-1, 1) and with --copyback 0 (the Frame's lists
// are what is filtered).  The installed lists are explicit, so every round searches like a first round: the temporal cache is lost.
// --reject_mode host|device (default host: the route above, unchanged): device hands the same masks to the search itself
// (Session::setRejectMasks -> mvicp_set_reject_mask, target side), once when a level's first round starts, and calls nothing per round: the
// lists stay searched lists, so the temporal cache, the list upkeep and the queued evaluations keep working, --copyback 1 is not needed, and
// with it on the frames receive the filtered lists through the ordinary copy-back.  No `boundary: round r dropped n pairs` lines.  The edge
// weight is the median over the kept pairs (host: over the unfiltered list), so the two modes' poses agree closely, not bit for bit.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>

#include "common_io.h"
#include "flags.h"
#include "frame.h"

using namespace mvicp;

static void loadFrames(const Flags& F, std::vector<std::shared_ptr<Frame>>& frames, const std::string& dir) {
  const std::vector<std::string> clouds = getAllTextFilesFromFolder(dir, "cloud");
  const std::vector<std::string> poses = getAllTextFilesFromFolder(dir, "pose");
  const std::vector<std::string> groundtruth = getAllTextFilesFromFolder(dir, "groundtruth");
  if (clouds.size() != poses.size()) std::cout << "unequal size" << std::endl;
  const int limit = F.i("limit", 40), step = F.i("step", 2);
  const double sigma = F.f("sigma", 0.02), sigmat = F.f("sigmat", 0.01);
  for (int i = 0; i < (int)clouds.size() && i < limit * step; i += step) {
    std::shared_ptr<Frame> f(new Frame());
    const int j = F.b("fake", false) ? 0 : i;
    loadXYZ(clouds[j], f->pts, f->nor, !F.b("drop_phantom_row", false));
    if (F.i("sor_k", 0) > 0) {
      const double radius = F.f("ror_radius", 0.0);
      const size_t before = f->pts.size();
      std::shared_ptr<Frame> kept = f->removeOutliers(F.i("sor_k", 0), F.f("sor_ratio", radius > 0.0 ? -1.0 : 2.0), radius);
      f->pts.swap(kept->pts); f->nor.swap(kept->nor); ++f->version;   // (a context that holds the old cloud re-uploads)
      std::cout << "outlier filter: frame " << frames.size() << " kept " << f->pts.size() << " of " << before << std::endl;
    }
    if (F.f("plane_tau", 0.0) > 0.0) {
      const size_t before = f->pts.size();
      double axis[3] = {0.0, 0.0, 0.0};
      const std::string ax = F.s("plane_axis", "");
      const bool has_axis = !ax.empty();
      if (has_axis && std::sscanf(ax.c_str(), "%lf,%lf,%lf", &axis[0], &axis[1], &axis[2]) != 3) { std::cerr << "--plane_axis needs x,y,z" << std::endl; std::exit(2); }
      const std::string keep = F.s("plane_keep", "rest");
      if (keep != "rest" && keep != "plane") { std::cerr << "--plane_keep needs rest or plane" << std::endl; std::exit(2); }
      mvicp_plane_result pr;
      std::shared_ptr<Frame> kept = f->removePlane(F.f("plane_tau", 0.0), std::atoll(F.s("plane_hyp", "1024").c_str()), std::strtoull(F.s("plane_seed", "0").c_str(), nullptr, 10),
                                                   has_axis ? axis : nullptr, F.f("plane_cos", 0.0), keep == "plane", &pr);
      f->pts.swap(kept->pts); f->nor.swap(kept->nor); ++f->version;   // (a context that holds the old cloud re-uploads)
      char line[256];
      std::snprintf(line, sizeof(line), "plane filter: frame %zu kept %zu of %zu, %d inliers, plane %.17g %.17g %.17g %.17g", frames.size(), f->pts.size(), before,
                    pr.count_refined, pr.normal[0], pr.normal[1], pr.normal[2], pr.d);
      std::cout << line << std::endl;
    }
    if (F.f("cluster_radius", 0.0) > 0.0) {
      const size_t before = f->pts.size();
      long long found = 0, stay = 0;
      std::shared_ptr<Frame> kept = f->removeSmallClusters(F.f("cluster_radius", 0.0), F.i("cluster_min_pts", 4), std::atoll(F.s("cluster_min_size", "0").c_str()),
                                                           std::atoll(F.s("cluster_keep", "0").c_str()), &found, &stay);
      f->pts.swap(kept->pts); f->nor.swap(kept->nor); ++f->version;   // (a context that holds the old cloud re-uploads)
      std::cout << "cluster filter: frame " << frames.size() << " kept " << f->pts.size() << " of " << before << ", " << stay << " of " << found << " clusters" << std::endl;
    }
    if (F.i("smooth_nn", 0) > 0) {
      std::vector<double> shift;
      std::vector<unsigned char> moved;
      for (int pass = 0; pass < F.i("smooth_iters", 1); ++pass) {
        std::shared_ptr<Frame> smooth = f->smoothPoints(F.i("smooth_nn", 0), F.f("smooth_radius", 0.0), F.i("smooth_degree", 2), F.f("smooth_max_shift", 0.0),
                                                        Vector3d(), &shift, &moved);
        f->pts.swap(smooth->pts); f->nor.swap(smooth->nor); ++f->version;   // (a context that holds the old cloud re-uploads)
      }
      size_t count = 0;
      double largest = 0.0;
      for (size_t j = 0; j < moved.size(); ++j) { count += moved[j]; largest = std::max(largest, std::fabs(shift[j])); }
      char line[160];
      std::snprintf(line, sizeof(line), "smooth: frame %zu moved %zu of %zu, largest |shift| %.17g", frames.size(), count, f->pts.size(), largest);
      std::cout << line << std::endl;
    }
    if (F.i("normals_nn", 0) > 0 && F.i("normals_fit", 0)) f->fitNormals(F.i("normals_nn", 0), F.f("normals_radius", 0.0), F.i("normals_fit", 0));
    else if (F.i("normals_nn", 0) > 0) f->estimateNormals(F.i("normals_nn", 0), F.f("normals_radius", 0.0));   // (viewpoint: the view's own origin)
    else if (F.b("recomputeNormals", true)) f->recomputeNormals();  // main_multiview.cpp:49,68-70 (default on)
    if (F.s("normals_orient", "") == "mst")
      std::cout << "normal orientation: frame " << frames.size() << " trees " << f->orientNormals(F.i("orient_nn", 10)) << std::endl;
    if (groundtruth.size() == clouds.size()) {
      f->pose = loadMatrix4d(poses[i]);
      f->poseGroundTruth = loadMatrix4d(groundtruth[i]);
    } else {
      f->poseGroundTruth = loadMatrix4d(poses[i]);
      f->pose = (i == 0) ? f->poseGroundTruth : addNoise(f->poseGroundTruth, sigma, sigmat);
    }
    frames.push_back(f);
  }
}

int main(int argc, char** argv) {
  Flags F(argc, argv);
  const bool pointToPlane = F.b("pointToPlane", true), sophusSE3 = F.b("sophusSE3", true), angleAxis = F.b("angleAxis", false);
  const bool robust = F.b("robust", true), quiet = F.b("quiet", false), symmetric = F.b("symmetric", false);
  const bool gicp = F.b("gicp", false);
  const double gicpEpsilon = F.f("gicp_epsilon", 1e-3);
  if (gicp && symmetric) { std::cerr << "--gicp and --symmetric name two objectives: give one" << std::endl; return 1; }
  const float cutoff = (float)F.f("cutoff", 0.05);
  const int knn = F.i("knn", 2), rounds = F.i("rounds", 20);
  const std::string dir = F.s("dir", "../samples/Bunny_RealData"), out = F.s("out", "");
  Session::get().device = F.i("device", 0);
  Session::get().copy_back = F.b("copyback", true);
  Session::get().copy_threads = F.i("copy_threads", 8);
  noiseStream() = F.s("noise_stream", "libstdc++") == "libc++" ? 1 : F.s("noise_stream", "libstdc++") == "g++" ? 2 : 0;

  if (!F.s("normals_orient", "").empty() && F.s("normals_orient", "") != "mst") { std::cerr << "--normals_orient must be mst" << std::endl; return 1; }
  if (F.i("normals_fit", 0) != 0 && F.i("normals_fit", 0) != 2 && F.i("normals_fit", 0) != 3) { std::cerr << "--normals_fit must be 2 or 3" << std::endl; return 1; }
  if (F.i("normals_fit", 0) != 0 && F.i("normals_nn", 0) <= 0) { std::cerr << "--normals_fit needs --normals_nn K" << std::endl; return 1; }
  for (const char* name : {"smooth_radius", "smooth_degree", "smooth_iters", "smooth_max_shift"})
    if (!F.s(name, "").empty() && F.i("smooth_nn", 0) <= 0) { std::cerr << "--" << name << " needs --smooth_nn K" << std::endl; return 1; }
  if (F.i("smooth_degree", 2) != 2 && F.i("smooth_degree", 2) != 3) { std::cerr << "--smooth_degree must be 2 or 3" << std::endl; return 1; }
  if (F.i("smooth_iters", 1) < 1) { std::cerr << "--smooth_iters must be at least 1" << std::endl; return 1; }
  const bool reject_boundary = F.b("reject_boundary", false);
  const int boundary_nn = F.i("boundary_nn", 30);
  const double boundary_radius = F.f("boundary_radius", 0.0), boundary_cos = F.f("boundary_cos", -0.5);
  if (reject_boundary && !(boundary_cos > -1.0 && boundary_cos < 1.0)) { std::cerr << "--boundary_cos must lie in (-1, 1)" << std::endl; return 1; }
  const std::string reject_mode = F.s("reject_mode", "host");
  if (reject_mode != "host" && reject_mode != "device") { std::cerr << "--reject_mode must be host or device" << std::endl; return 1; }
  const bool reject_device = reject_boundary && reject_mode == "device";
  if (reject_boundary && !reject_device && !Session::get().copy_back) { std::cerr << "--reject_boundary filters the frames' lists: it needs --copyback 1" << std::endl; return 1; }
  std::vector<std::shared_ptr<Frame>> frames;
  try {
    loadFrames(F, frames, dir);
  } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
  if (frames.empty()) { std::cerr << "no frames loaded from " << dir << std::endl; return 1; }
  if (!F.s("dump_knn", "").empty()) {
    try {
      const size_t k = (size_t)F.i("knn_k", 10);
      std::ofstream f(F.s("dump_knn", "").c_str(), std::ios::binary);
      for (int i = 0; i < (int)frames[0]->pts.size(); ++i) {
        const std::vector<Vector3d> nb = frames[0]->getNeighbours(i, k);
        for (const Vector3d& p : nb) f.write(reinterpret_cast<const char*>(p.data()), 24);
      }
    } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
    return 0;
  }
  if (F.s("init", "") == "features") {
    try {
      Session::FeatureInit o;
      o.voxel = F.f("feat_voxel", 0.0);
      o.radius = F.f("feat_radius", 5.0 * o.voxel); o.tau = F.f("feat_tau", 1.5 * o.voxel);
      o.max_nn = F.i("feat_max_nn", 64); o.min_count = F.i("feat_min_count", 3);
      o.hypotheses = std::atoll(F.s("feat_hyp", "10000").c_str());
      o.edge_sim = F.f("feat_edge_sim", 0.9);
      o.seed = std::strtoull(F.s("feat_seed", "0").c_str(), nullptr, 10);
      o.refine = F.b("feat_refine", true);
      const std::string kp = F.s("feat_keypoints", "none");
      if (kp != "none" && kp != "iss" && kp != "iss_src") { std::cerr << "--feat_keypoints must be none, iss or iss_src" << std::endl; return 1; }
      o.keypoints = kp == "iss" ? 1 : kp == "iss_src" ? 2 : 0;
      o.salient_radius = F.f("feat_salient_radius", o.radius); o.nms_radius = F.f("feat_nms_radius", 0.3 * o.salient_radius);
      o.gamma21 = F.f("feat_gamma21", 0.975); o.gamma32 = F.f("feat_gamma32", 0.975); o.min_neighbors = F.i("feat_min_neighbors", 5);
      std::vector<Session::FeatureEdge> fe;
      std::vector<Session::FeatureKeypoints> kc;
      const int comps = Session::get().initFromFeatures(frames, o, &fe, &kc);
      for (size_t i = 0; i < kc.size(); ++i)
        std::cout << "feature init: frame " << i << " keypoints " << kc[i].keypoints << " of " << kc[i].points << std::endl;
      for (const Session::FeatureEdge& e : fe)
        std::cout << "feature init: edge " << e.src << " " << e.dst << " pairs " << e.pairs << " accepted " << e.accepted << " inliers " << e.inliers << std::endl;
      std::cout << "feature init: " << comps << " component(s)" << std::endl;
    } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
  }
  frames[0]->fixed = true;
  const bool overlap_graph = F.s("graph", "pose") == "overlap";
  int components = 0;
  try {
    if (overlap_graph)
      components = Session::get().computeOverlapNeighbours(frames, knn, (float)F.f("overlap_cutoff", cutoff), F.i("overlap_samples", 4096), F.f("overlap_min", 0.0));
    else
      for (int i = 0; i < (int)frames.size(); ++i) frames[i]->computePoseNeighboursKnn(&frames, i, knn);
  } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
  if (!quiet) {
    std::cout << "graph adjacency matrix == block structure" << std::endl;
    for (size_t i = 0; i < frames.size(); ++i) {
      std::vector<int> row(frames.size(), 0);
      for (const OutgoingEdge& e : frames[i]->neighbours) row[e.neighbourIdx] = 1;
      for (int v : row) std::cout << v << " ";
      std::cout << std::endl;
    }
    if (overlap_graph) std::cout << "overlap graph: " << components << " component(s)" << std::endl;
  }
  if (F.s("normals_orient", "") == "mst" && frames.size() > 1) {
    try {
      std::vector<unsigned char> flipped;
      const int comps = Session::get().orientFrames(frames, cutoff, 0, &flipped);
      std::cout << "normal orientation: " << comps << " component(s), flipped";
      for (unsigned char f : flipped) std::cout << " " << (int)f;
      std::cout << std::endl;
    } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
  }
  const int coarse_rounds = F.i("coarse_rounds", 0);
  std::vector<std::shared_ptr<Frame>> coarse;   // the frames' voxelDownsample copies (coarse_rounds > 0)
  if (coarse_rounds > 0) {
    try {
      // all clouds into the session first: voxelDownsample then finds every frame there (Session::query_context) instead of uploading the
      // frames one after the other into a context of their own, each waiting for the previous one's structure build
      Session::get().ensure_uploaded(frames);
      for (auto& f : frames) coarse.push_back(f->voxelDownsample(F.f("coarse_voxel", 0.0)));
    } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
    if (!quiet)
      for (size_t i = 0; i < frames.size(); ++i) std::cout << "coarse frame " << i << ": " << coarse[i]->pts.size() << " of " << frames[i]->pts.size() << " points" << std::endl;
  }
  std::vector<std::vector<unsigned char>> masks, coarse_masks;   // --reject_boundary: one byte per point of every frame (and of every coarse copy)
  if (reject_boundary) {
    for (size_t i = 0; i < frames.size(); ++i)
      if (frames[i]->nor.size() != frames[i]->pts.size()) { std::cerr << "--reject_boundary: frame " << i << " has no normals" << std::endl; return 1; }
    try {
      Session::get().ensure_uploaded(frames);   // (every frame is found in the session: no context of its own per frame)
      for (size_t i = 0; i < frames.size(); ++i) {
        masks.push_back(frames[i]->boundaryPoints(boundary_nn, boundary_radius, boundary_cos));
        size_t flagged = 0;
        for (unsigned char b : masks[i]) flagged += b;
        std::cout << "boundary: frame " << i << " flagged " << flagged << " of " << masks[i].size() << std::endl;
      }
      for (auto& f : coarse) coarse_masks.push_back(f->boundaryPoints(boundary_nn, boundary_radius, boundary_cos));
    } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
  }
  auto poses_to_full = [&]() { for (size_t i = 0; i < coarse.size(); ++i) frames[i]->pose = coarse[i]->pose; };
  double wall_search = 0.0, wall_solve = 0.0;
  std::ofstream trace;
  if (!F.s("trace", "").empty()) { trace.open(F.s("trace", "").c_str()); trace.precision(17); }
  try {
    for (int r = 0; r < rounds; ++r) {
      if (r == coarse_rounds && !coarse.empty()) poses_to_full();
      std::vector<std::shared_ptr<Frame>>& cur = r < coarse_rounds ? coarse : frames;   // this round's level
      // --reject_mode device: the level's masks go to the device once, when its first round starts; nothing is called per round
      if (reject_device && (r == 0 || r == coarse_rounds)) Session::get().setRejectMasks(cur, r < coarse_rounds ? coarse_masks : masks, MVICP_REJECT_AS_TARGET);
      if (r == F.i("perturb_round", -1) && F.i("perturb_frame", -1) >= 0 && F.i("perturb_frame", -1) < (int)cur.size())
        cur[F.i("perturb_frame", -1)]->pose.m[12] += 1e-4;
      const unsigned long long c0 = Session::get().edges_copied, s0 = Session::get().edges_skipped;
      const auto t0 = std::chrono::steady_clock::now();
      for (auto& f : cur) f->computeClosestPointsToNeighbours(&cur, cutoff);
      if (reject_boundary && !reject_device) {
        long long total = 0;
        for (long long d : Session::get().rejectBoundary(cur, r < coarse_rounds ? coarse_masks : masks)) total += d;
        std::cout << "boundary: round " << r << " dropped " << total << " pairs" << std::endl;
      }
      const auto t1 = std::chrono::steady_clock::now();
      if (trace.is_open())
        for (size_t i = 0; i < cur.size(); ++i)
          for (size_t j = 0; j < cur[i]->neighbours.size(); ++j) {
            const OutgoingEdge& e = cur[i]->neighbours[j];
            unsigned int bits;
            std::memcpy(&bits, &e.weight, 4);
            trace << "C " << r << " " << i << " " << j << " " << e.neighbourIdx << " " << e.correspondances.size() << " " << bits << "\n";
          }
      if (F.b("copy_stats", false))
        std::cout << "copyback: round " << r << " copied " << Session::get().edges_copied - c0 << " skipped " << Session::get().edges_skipped - s0 << std::endl;
      if (r == rounds - 1 && !F.s("dump_corr", "").empty()) {
        for (size_t i = 0; i < cur.size(); ++i) saveMatrix4d(F.s("dump_corr", "") + "/search_pose_" + std::to_string(i) + ".txt", cur[i]->pose);
        for (size_t i = 0; i < cur.size(); ++i)
          for (size_t j = 0; j < cur[i]->neighbours.size(); ++j) {
            const OutgoingEdge& e = cur[i]->neighbours[j];
            std::ofstream f((F.s("dump_corr", "") + "/corr_" + std::to_string(i) + "_" + std::to_string(j) + ".txt").c_str());
            f.precision(17);
            f << e.neighbourIdx << " " << e.weight << " " << e.correspondances.size() << "\n";
            for (const Correspondance& c : e.correspondances) f << c.first << " " << c.second << " " << c.dist << "\n";
          }
      }
      if (r == rounds - 1 && F.i("check_nn", 0) > 0) {
        // S1' through the Frame mirror: q = dst.pose^-1 * (src.pose * p) (frame.cpp:131,136) -> dst.getClosestPoint(q) must give
        // the correspondence's neighbour and distance
        long checked = 0, bad = 0, single = 0;
        for (size_t i = 0; i < cur.size(); ++i)
          for (const OutgoingEdge& e : cur[i]->neighbours) {
            Frame& d = *cur[e.neighbourIdx];
            const Isometry3d M = d.pose.inverse() * cur[i]->pose;
            const int n = std::min<int>(F.i("check_nn", 0), (int)e.correspondances.size());
            // the batched form (one launch for the edge's queries) ...
            std::vector<Vector3d> qs(n);
            for (int k = 0; k < n; ++k) qs[k] = M * cur[i]->pts[e.correspondances[k].first];
            std::vector<size_t> idxs;
            const std::vector<double> d2s = d.getClosestPoints(qs, idxs);
            for (int k = 0; k < n; ++k) {
              const Correspondance& c = e.correspondances[k];
              ++checked;
              if ((int)idxs[k] != c.second || std::fabs(std::sqrt(d2s[k]) - c.dist) > 1e-12) ++bad;
              if (k < 8) {   // ... and the reference's one-query signature on a few of them: identical answers
                size_t idx = 0;
                const double d2 = d.getClosestPoint(qs[k], idx);
                ++single;
                if (idx != idxs[k] || d2 != d2s[k]) ++bad;
              }
            }
          }
        std::cout << "getClosestPoint check: " << checked << " queries, " << bad << " mismatches (" << single << " also asked one by one)" << std::endl;
      }
      if (F.i("freeze_from", 1 << 30) <= r) {}   // (search only: the poses stay bit-identical)
      else if (gicp)
        Session::get().optimizeGicp(cur, sophusSE3 ? MVICP_PARAM_SOPHUS_SE3 : angleAxis ? MVICP_PARAM_ANGLE_AXIS : MVICP_PARAM_EIGEN_QUATERNION, gicpEpsilon, robust);
      else if (symmetric)
        Session::get().optimize(cur, sophusSE3 ? MVICP_PARAM_SOPHUS_SE3 : angleAxis ? MVICP_PARAM_ANGLE_AXIS : MVICP_PARAM_EIGEN_QUATERNION, MVICP_METRIC_SYMMETRIC, robust);
      else if (sophusSE3) ICP_Ceres::ceresOptimizer_sophusSE3(cur, pointToPlane, robust);
      else if (angleAxis) ICP_Ceres::ceresOptimizer_ceresAngleAxis(cur, pointToPlane, robust);
      else ICP_Ceres::ceresOptimizer(cur, pointToPlane, robust);
      const auto t2 = std::chrono::steady_clock::now();
      if (trace.is_open())
        for (size_t i = 0; i < cur.size(); ++i) {
          trace << "P " << r << " " << i;
          for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) trace << " " << cur[i]->pose.m[a + 4 * b];
          trace << "\n";
        }
      wall_search += std::chrono::duration<double, std::milli>(t1 - t0).count();
      wall_solve += std::chrono::duration<double, std::milli>(t2 - t1).count();
      if (!quiet)
        std::cout << "round: " << r << "  closest pts " << std::chrono::duration<double, std::milli>(t1 - t0).count() << " ms  global "
                  << std::chrono::duration<double, std::milli>(t2 - t1).count() << " ms" << std::endl;
    }
  } catch (const std::exception& ex) {
    std::cerr << ex.what() << std::endl;
    return 2;
  }
  if (coarse_rounds >= rounds && rounds > 0 && !coarse.empty()) poses_to_full();   // (every round ran on the coarse level)
  // whole-loop wall clock of the drop-in route (Frame API + session + copy-back): parsed by bench.py / tools/dropin_bench.py
  std::cout << "loop: rounds " << rounds << " copyback " << (Session::get().copy_back ? 1 : 0) << " closest_pts_ms " << wall_search << " global_ms " << wall_solve
            << " it_per_s " << (rounds > 0 ? 1e3 * rounds / (wall_search + wall_solve) : 0.0) << std::endl;
  for (size_t i = 0; i < frames.size(); ++i) {
    if (!quiet) std::cout << "frame " << i << poseDiff(frames[i]->pose, frames[i]->poseGroundTruth);
    if (!out.empty()) saveMatrix4d(out + "/pose_" + std::to_string(i) + ".txt", frames[i]->pose);
  }
  if (!F.s("fused_out", "").empty()) {
    try {
      std::vector<Vector3d> fp, fn;
      const long long m = Session::get().fusedModel(frames, F.f("fused_voxel", 0.0), fp, fn);
      std::ofstream f(F.s("fused_out", "").c_str());
      f.precision(17);
      for (long long v = 0; v < m; ++v) {
        f << fp[v][0] << " " << fp[v][1] << " " << fp[v][2];
        if (!fn.empty()) f << " " << fn[v][0] << " " << fn[v][1] << " " << fn[v][2];
        f << "\n";
      }
      if (!quiet) std::cout << "fused model: " << m << " voxels" << std::endl;
    } catch (const std::exception& ex) { std::cerr << ex.what() << std::endl; return 2; }
  }
  Session::get().reset();
  return 0;
}
