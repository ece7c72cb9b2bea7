// Implementation of the Frame / ICP_Ceres mirror (host/frame.h) over the C ABI.
#include "frame.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <stdexcept>
#include <thread>

namespace mvicp {

static void check(int st) {
  if (st < 0) throw std::runtime_error(std::string("mvicp: ") + mvicp_last_error());
}

// a refused call's message, taken before any further library call (a clean-up call may overwrite the thread's message)
static std::string failure(int st) { return st < 0 ? std::string("mvicp: ") + mvicp_last_error() : std::string(); }

Session& Session::get() {
  static Session* s = new Session();   // never destroyed: ~Frame() of a Frame with static lifetime may still ask for it during exit
  return *s;
}

void Session::reset() {
  if (ctx) mvicp_destroy(ctx);
  if (side_ctx) mvicp_destroy(side_ctx);
  ctx = nullptr; side_ctx = nullptr; side_owner = nullptr; side_key = FrameKey{nullptr, nullptr, 0, nullptr, 0};
  frames_key = nullptr;
  frame_keys.clear();
  last_poses.clear();
  graph_bound = false;
  esrc.clear(); edst.clear();
  held.clear(); epochs = nullptr; corr = nullptr; corr_off = nullptr;   // (they pointed into the context that has just ended)
  reject_masks.clear(); reject_roles = 0; reject_key = nullptr;
  ++knn_generation;
}

void Session::invalidate() {
  invalidate_lists();
  frames_key = nullptr;
  frame_keys.clear();
  last_poses.clear();
  side_owner = nullptr;
  ++knn_generation;
}

void Session::forget(const Frame* f) {
  if (side_owner == f) side_owner = nullptr;
  if (frame_index(f) >= 0) { frames_key = nullptr; frame_keys.clear(); last_poses.clear(); }   // the next bind uploads; the lists' bookkeeping is per edge and stays
}

Frame::~Frame() { Session::get().forget(this); }

int Session::frame_index(const Frame* f) const {
  for (size_t i = 0; i < frame_keys.size(); ++i) if (frame_keys[i].f == f) return (int)i;
  return -1;
}

static std::vector<Session::FrameKey> frame_keys_of(const std::vector<std::shared_ptr<Frame>>& frames) {
  std::vector<Session::FrameKey> keys(frames.size());
  for (size_t i = 0; i < frames.size(); ++i) {
    const Frame& f = *frames[i];
    keys[i] = Session::FrameKey{&f, f.pts.empty() ? nullptr : (const void*)f.pts[0].data(), f.pts.size(), f.nor.empty() ? nullptr : (const void*)f.nor[0].data(), f.version};
  }
  return keys;
}

void Session::upload(std::vector<std::shared_ptr<Frame>>& frames) {
  // mvicp_set_num_frames drops every cloud and the graph: from here until the caller records the new keys the session holds nothing it
  // could take for current, whichever call below throws
  frames_key = nullptr; frame_keys.clear(); graph_bound = false; esrc.clear(); edst.clear();
  last_poses.clear(); held.clear(); epochs = nullptr; corr = nullptr; corr_off = nullptr;
  if (!ctx) check(mvicp_create(device, &ctx));
  check(mvicp_set_num_frames(ctx, (int)frames.size()));
  for (size_t i = 0; i < frames.size(); ++i) {
    Frame& f = *frames[i];
    const double* nrm = f.nor.size() == f.pts.size() && !f.nor.empty() ? f.nor[0].data() : nullptr;
    check(mvicp_set_frame(ctx, (int)i, f.pts.empty() ? nullptr : f.pts[0].data(), nrm, (int)f.pts.size()));
  }
  install_reject_masks(frames);   // (mvicp_set_num_frames dropped them with the clouds; no-op unless setRejectMasks was given this vector)
}

void Session::bind(std::vector<std::shared_ptr<Frame>>& frames) {
  // graph in the reference's loop order: src ascending, neighbour order (main_multiview.cpp:119-127)
  std::vector<int> s, d;
  for (size_t i = 0; i < frames.size(); ++i)
    for (const OutgoingEdge& e : frames[i]->neighbours) { s.push_back((int)i); d.push_back(e.neighbourIdx); }
  const std::vector<FrameKey> keys = frame_keys_of(frames);
  const bool same_frames = ctx && frames_key == (const void*)&frames && keys == frame_keys;
  if (same_frames && graph_bound && s == esrc && d == edst) return;
  if (!(same_frames && !graph_bound)) upload(frames);   // (clouds that computeOverlapNeighbours has just uploaded are not uploaded again)
  check(mvicp_set_graph(ctx, (int)s.size(), s.data(), d.data()));
  esrc = s; edst = d;
  graph_bound = true;
  frames_key = (const void*)&frames;
  frame_keys = keys;
  last_poses.clear();
  held.assign(esrc.size(), Held());
  epochs = nullptr;
}

void Session::ensure_uploaded(std::vector<std::shared_ptr<Frame>>& frames) {
  const std::vector<FrameKey> keys = frame_keys_of(frames);
  if (ctx && frames_key == (const void*)&frames && keys == frame_keys) return;
  upload(frames);
  frames_key = (const void*)&frames; frame_keys = keys;
  graph_bound = false; esrc.clear(); edst.clear();
  last_poses.clear(); held.clear(); epochs = nullptr; corr = nullptr; corr_off = nullptr;
}

long long Session::fusedModel(std::vector<std::shared_ptr<Frame>>& frames, double voxel, std::vector<Vector3d>& pts, std::vector<Vector3d>& nor) {
  ensure_uploaded(frames);
  std::vector<double> P(16 * frames.size());
  for (size_t i = 0; i < frames.size(); ++i) std::memcpy(&P[16 * i], frames[i]->pose.data(), 128);
  int has_normals = 0;
  const long long m = mvicp_voxel_grid(ctx, 0, nullptr, P.data(), voxel, &has_normals);
  if (m < 0) check((int)m);
  pts.assign((size_t)m, Vector3d());
  nor.assign(has_normals ? (size_t)m : 0, Vector3d());
  if (m) check(mvicp_voxel_fetch(ctx, m, pts[0].data(), has_normals ? nor[0].data() : nullptr, nullptr));
  return m;
}

int Session::computeOverlapNeighbours(std::vector<std::shared_ptr<Frame>>& frames, int knn, float thresh, int max_samples, double min_fraction) {
  const int K = (int)frames.size();
  ensure_uploaded(frames);
  std::vector<double> P(16 * (size_t)K);
  for (int i = 0; i < K; ++i) std::memcpy(&P[16 * (size_t)i], frames[i]->pose.data(), 128);
  std::vector<int> samples(K), hits((size_t)K * K), src((size_t)K * K), dst((size_t)K * K);
  std::vector<long long> sumq((size_t)K * K);
  check(mvicp_overlap(ctx, P.data(), thresh, max_samples, samples.data(), hits.data(), sumq.data(), nullptr));
  int comps = 0;
  const int E = mvicp_graph_from_overlap(K, samples.data(), hits.data(), sumq.data(), knn, min_fraction, 0, K * K, src.data(), dst.data(), &comps);
  check(E);
  for (auto& f : frames) f->neighbours.clear();
  for (int e = 0; e < E; ++e) {
    const int i = src[e], j = dst[e];
    const float fraction = (float)((double)hits[(size_t)i * K + j] / (double)samples[i]);
    frames[i]->neighbours.push_back(OutgoingEdge{j, 1.f - fraction, {}});   // "smaller is nearer" holds until the first search overwrites it
  }
  return comps;
}

int Session::initFromFeatures(std::vector<std::shared_ptr<Frame>>& frames, const FeatureInit& o, std::vector<FeatureEdge>* edges_out,
                              std::vector<FeatureKeypoints>* keypoint_counts) {
  const int K = (int)frames.size();
  if (edges_out) edges_out->clear();
  if (keypoint_counts) keypoint_counts->clear();
  if (K < 1) return 0;
  // the clouds that carry the features: the frames themselves or their voxel copies
  std::vector<std::shared_ptr<Frame>> feat;
  // (with voxel > 0 the session holds the copies, which end with this call -- also when it throws: the next bind uploads the frames)
  struct Forget { Session* s; bool on; ~Forget() { if (on) s->invalidate(); } } forget_copies{this, o.voxel > 0.0};
  if (o.voxel > 0.0) {
    ensure_uploaded(frames);   // (voxelDownsample then finds every frame in the session)
    for (auto& f : frames) feat.push_back(f->voxelDownsample(o.voxel));
  }
  std::vector<std::shared_ptr<Frame>>& carry = o.voxel > 0.0 ? feat : frames;
  ensure_uploaded(carry);
  std::vector<long long> offsets((size_t)K + 1, 0);
  for (int i = 0; i < K; ++i) offsets[i + 1] = offsets[i] + (long long)carry[i]->pts.size();
  const size_t total = (size_t)offsets[K];
  std::vector<double> desc(33 * total), xyz(3 * total);
  for (int i = 0; i < K; ++i) {
    const size_t n = carry[i]->pts.size();
    if (n) std::memcpy(&xyz[3 * (size_t)offsets[i]], carry[i]->pts[0].data(), 24 * n);
    const long long got = mvicp_fpfh(ctx, i, o.radius, o.max_nn);
    if (got < 0) check((int)got);
    if (n) check(mvicp_fpfh_fetch(ctx, (long long)n, &desc[33 * (size_t)offsets[i]], nullptr));
  }
  std::vector<int> src, dst;
  for (int i = 0; i < K; ++i)
    for (int j = i + 1; j < K; ++j) { src.push_back(i); dst.push_back(j); }
  const int E = (int)src.size();
  int n_sets = K;
  std::vector<int> set_dst = dst;   // the set an edge's destination rows come from
  if (o.keypoints) {
    // the keypoint rows of every frame, gathered in front of (2: the source side only) or instead of (1) the full sets
    std::vector<long long> k_off((size_t)K + 1, 0);
    std::vector<double> k_desc, k_xyz;
    for (int i = 0; i < K; ++i) {
      const long long k = mvicp_iss_keypoints(ctx, i, o.salient_radius, o.nms_radius, o.gamma21, o.gamma32, o.min_neighbors);
      if (k < 0) check((int)k);
      std::vector<int> idx((size_t)k);
      if (k) check(mvicp_iss_fetch(ctx, k, idx.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr));
      for (int r : idx) {
        const size_t row = (size_t)offsets[i] + (size_t)r;
        k_desc.insert(k_desc.end(), &desc[33 * row], &desc[33 * row] + 33);
        k_xyz.insert(k_xyz.end(), &xyz[3 * row], &xyz[3 * row] + 3);
      }
      k_off[i + 1] = k_off[i] + k;
      if (keypoint_counts) keypoint_counts->push_back(FeatureKeypoints{(int)k, (int)carry[i]->pts.size()});
    }
    if (o.keypoints == 2) {
      for (int i = 1; i <= K; ++i) k_off.push_back(k_off[K] + offsets[i]);
      k_desc.insert(k_desc.end(), desc.begin(), desc.end());
      k_xyz.insert(k_xyz.end(), xyz.begin(), xyz.end());
      for (int& d : set_dst) d += K;
      n_sets = 2 * K;
    }
    offsets.swap(k_off); desc.swap(k_desc); xyz.swap(k_xyz);
  }
  std::vector<unsigned long long> seeds((size_t)E);
  for (int e = 0; e < E; ++e) seeds[e] = o.seed + (unsigned long long)e;
  std::vector<mvicp_coarse_edge> res((size_t)E);
  const long long st = mvicp_coarse_pairs(ctx, desc.data(), xyz.data(), offsets.data(), n_sets, 33, E, src.data(), set_dst.data(), seeds.data(), 1, 1.0, o.hypotheses,
                                          o.tau, o.edge_sim, res.data());
  if (st < 0) check((int)st);
  std::vector<int> count((size_t)E);
  std::vector<double> pose(16 * (size_t)E);
  for (int e = 0; e < E; ++e) {
    count[e] = res[e].count;
    std::memcpy(&pose[16 * (size_t)e], res[e].pose, 128);
    if (o.refine && res[e].count >= 3) {
      const size_t c = (size_t)res[e].pairs;
      std::vector<int> pairs(2 * c);
      std::vector<unsigned char> flags(c);
      check(mvicp_coarse_pairs_fetch(ctx, e, (long long)c, pairs.data(), flags.data()));
      std::vector<double> P, Q;
      for (size_t k = 0; k < c; ++k)
        if (flags[k]) {
          const double* p = &xyz[3 * ((size_t)offsets[src[e]] + (size_t)pairs[2 * k])];
          const double* q = &xyz[3 * ((size_t)offsets[set_dst[e]] + (size_t)pairs[2 * k + 1])];
          P.insert(P.end(), p, p + 3); Q.insert(Q.end(), q, q + 3);
        }
      check(mvicp_closedform_point_to_point(P.data(), Q.data(), (int)(P.size() / 3), &pose[16 * (size_t)e]));
    }
    if (edges_out) edges_out->push_back(FeatureEdge{src[e], dst[e], res[e].pairs, res[e].accepted, res[e].count});
  }
  std::vector<double> out(16 * (size_t)K);
  const int comps = mvicp_poses_from_pairs(K, E, src.data(), dst.data(), count.data(), pose.data(), o.min_count, 0, frames[0]->pose.data(), out.data(), nullptr,
                                           nullptr, nullptr);
  check(comps);
  for (int i = 1; i < K; ++i) std::memcpy(frames[i]->pose.data(), &out[16 * (size_t)i], 128);
  return comps;
}

void Session::correspond(std::vector<std::shared_ptr<Frame>>& frames, float thresh) {
  bind(frames);
  std::vector<double> P(16 * frames.size());
  std::vector<unsigned char> fx(frames.size());
  for (size_t i = 0; i < frames.size(); ++i) { std::memcpy(&P[16 * i], frames[i]->pose.data(), 128); fx[i] = frames[i]->fixed; }
  if (P == last_poses && thresh == last_thresh && fx == last_fixed && nn_method == last_nn_method) {
    // same round: the batched result is still valid.  (copy_back switched on since that search: its lists were never mapped)
    if (copy_back && !corr) {
      check(mvicp_map_correspondences_async(ctx, &corr, &corr_off));
      check(mvicp_correspondence_epochs(ctx, &epochs));
    }
    return;
  }
  last_poses.clear();   // (a refused search leaves no cached round behind)
  corr = nullptr; corr_off = nullptr;
  counts.assign(esrc.size(), 0);
  weights.assign(esrc.size(), 0.f);
  check(mvicp_correspond(ctx, P.data(), fx.data(), thresh, nn_method, counts.data(), weights.data()));
  last_poses = P;
  last_thresh = thresh;
  last_fixed = fx;
  last_nn_method = nn_method;
  // the literal drop-in contract: every list in the reference's layout, un-sorted on the device, ONE copy per round for all edges
  if (copy_back) {
    check(mvicp_map_correspondences_async(ctx, &corr, &corr_off));   // (no device work when the search reproduced every list: mvicp.h); chunks arrive frame by frame
    check(mvicp_correspondence_epochs(ctx, &epochs));
  }
}

std::vector<long long> Session::rejectBoundary(std::vector<std::shared_ptr<Frame>>& frames, const std::vector<std::vector<unsigned char>>& masks) {
  if (!ctx || !graph_bound || last_poses.empty()) throw std::runtime_error("mvicp: rejectBoundary needs the round's search before it");
  if (!copy_back) throw std::runtime_error("mvicp: rejectBoundary filters the Frame's lists: it needs copy_back");
  if (masks.size() != frames.size()) throw std::runtime_error("mvicp: rejectBoundary needs one mask per frame");
  for (size_t j = 0; j < frames.size(); ++j)
    if (!masks[j].empty() && masks[j].size() != frames[j]->pts.size()) throw std::runtime_error("mvicp: rejectBoundary: a mask has one byte per point of its frame");
  std::vector<long long> dropped;
  std::vector<int> first, second;
  bool any = false;
  size_t e = 0;
  for (size_t i = 0; i < frames.size(); ++i) {
    Frame& f = *frames[i];
    for (OutgoingEdge& edge : f.neighbours) {
      const std::vector<unsigned char>& m = masks[(size_t)edge.neighbourIdx];
      std::vector<Correspondance>& L = edge.correspondances;
      size_t w = 0;
      if (!f.fixed && !m.empty()) {   // (a fixed frame is not searched: computeClosestPointsToNeighbours left its lists alone)
        for (size_t r = 0; r < L.size(); ++r)
          if (!m[(size_t)L[r].second]) L[w++] = L[r];
      } else {
        w = L.size();
      }
      const long long d = (long long)(L.size() - w);
      if (d) {
        L.resize(w);
        first.resize(w); second.resize(w);
        for (size_t r = 0; r < w; ++r) { first[r] = L[r].first; second[r] = L[r].second; }
        check(mvicp_set_correspondences(ctx, (int)e, (int)w, first.data(), second.data(), weights[e]));
        if (e < held.size()) held[e] = Held();   // (the library's list has a new epoch and the Frame's vector is not a copy of the mapped triples)
        any = true;
      }
      dropped.push_back(d);
      ++e;
    }
  }
  // an installed list ends the mapped triples and the cached round: the next correspond() searches again and maps anew
  if (any) { last_poses.clear(); corr = nullptr; corr_off = nullptr; }
  return dropped;
}

void Session::install_reject_masks(const std::vector<std::shared_ptr<Frame>>& frames) {
  if (reject_key != (const void*)&frames || reject_masks.size() != frames.size()) return;   // (masks of another frames vector: not these clouds')
  for (size_t j = 0; j < frames.size(); ++j) {
    const std::vector<unsigned char>& m = reject_masks[j];
    if (!m.empty() && m.size() != frames[j]->pts.size()) throw std::runtime_error("mvicp: setRejectMasks: a mask has one byte per point of its frame");
    check(mvicp_set_reject_mask(ctx, (int)j, m.empty() ? nullptr : m.data(), reject_roles));
  }
}

void Session::setRejectMasks(std::vector<std::shared_ptr<Frame>>& frames, const std::vector<std::vector<unsigned char>>& masks, int roles) {
  if (masks.size() != frames.size()) throw std::runtime_error("mvicp: setRejectMasks needs one mask per frame");
  if (roles < 0 || roles > 3) throw std::runtime_error("mvicp: setRejectMasks: roles outside [0, 3]");
  for (size_t j = 0; j < frames.size(); ++j)
    if (!masks[j].empty() && masks[j].size() != frames[j]->pts.size()) throw std::runtime_error("mvicp: setRejectMasks: a mask has one byte per point of its frame");
  reject_masks = masks; reject_roles = roles; reject_key = (const void*)&frames;
  // into the context now if it holds exactly these clouds; otherwise the upload that brings them installs the masks
  if (ctx && frames_key == (const void*)&frames && frame_keys_of(frames) == frame_keys) install_reject_masks(frames);
  last_poses.clear(); corr = nullptr; corr_off = nullptr;   // (a cached round was searched under the old masks)
}

void Session::optimize(std::vector<std::shared_ptr<Frame>>& frames, int param, bool pointToPlane, bool robust, mvicp_summary* out) {
  optimize(frames, param, pointToPlane ? MVICP_METRIC_PLANE : MVICP_METRIC_POINT, robust, out);
}

void Session::optimize(std::vector<std::shared_ptr<Frame>>& frames, int param, mvicp_metric metric, bool robust, mvicp_summary* out) {
  bind(frames);
  std::vector<double> P(16 * frames.size());
  std::vector<unsigned char> fx(frames.size());
  for (size_t i = 0; i < frames.size(); ++i) { std::memcpy(&P[16 * i], frames[i]->pose.data(), 128); fx[i] = frames[i]->fixed; }
  mvicp_summary sm;
  check(mvicp_optimize_metric(ctx, P.data(), fx.data(), param, metric, robust, 50 /* icp-ceres.cpp:81 */, &sm));
  if (!frames.empty()) frames[0]->fixed = true;  // icp-ceres.cpp:244,341,417
  for (size_t i = 0; i < frames.size(); ++i) std::memcpy(frames[i]->pose.data(), &P[16 * i], 128);
  if (out) *out = sm;
}

void Session::optimizeGicp(std::vector<std::shared_ptr<Frame>>& frames, int param, double epsilon, bool robust, mvicp_summary* out) {
  bind(frames);
  std::vector<double> P(16 * frames.size());
  std::vector<unsigned char> fx(frames.size());
  for (size_t i = 0; i < frames.size(); ++i) { std::memcpy(&P[16 * i], frames[i]->pose.data(), 128); fx[i] = frames[i]->fixed; }
  mvicp_summary sm;
  check(mvicp_optimize_gicp(ctx, P.data(), fx.data(), param, epsilon, robust, 50 /* icp-ceres.cpp:81 */, &sm));
  if (!frames.empty()) frames[0]->fixed = true;  // icp-ceres.cpp:244,341,417
  for (size_t i = 0; i < frames.size(); ++i) std::memcpy(frames[i]->pose.data(), &P[16 * i], 128);
  if (out) *out = sm;
}

void Frame::computePoseNeighboursKnn(std::vector<std::shared_ptr<Frame>>* frames, int i, int k) {
  neighbours.clear();
  const Vector3d t1 = pose.translation();
  for (int j = 0; j < (int)frames->size(); ++j) {
    if (i == j) continue;
    const float diff_tra = (float)(t1 - (*frames)[j]->pose.translation()).norm();
    neighbours.push_back(OutgoingEdge{j, diff_tra, {}});
  }
  auto less = [](const OutgoingEdge& a, const OutgoingEdge& b) { return a.weight < b.weight; };
  if ((int)neighbours.size() < k) {
    std::sort(neighbours.begin(), neighbours.end(), less);
  } else {
    std::partial_sort(neighbours.begin(), neighbours.begin() + k, neighbours.end(), less);
    neighbours.resize(k);
  }
}

// dst[i] <- src[i] for a few (destination, source, bytes) pieces on up to `threads` host threads: a frame's lists are a few megabytes
// each; one thread copies at ~5 GB/s, the memory system takes eight such streams.  The workers are PERSISTENT (created on first use, parked
// on a condition variable): a driver calls this once per frame per round, and creating eight threads per call cost more than the copy.
namespace {
struct CopyJob { char* d; const char* s; size_t n; };
class CopyPool {
 public:
  static CopyPool& get() { static CopyPool p; return p; }
  void run(const std::vector<CopyJob>& jobs, int threads) {
    const int nt = (int)std::min<size_t>((size_t)std::max(1, threads), jobs.size());
    if (nt <= 1) { for (const CopyJob& j : jobs) std::memcpy(j.d, j.s, j.n); return; }
    std::unique_lock<std::mutex> lk(m_);
    while ((int)workers_.size() < nt - 1) workers_.emplace_back([this]() { loop(); });
    jobs_ = &jobs; next_.store(0); pending_ = (int)workers_.size(); ++epoch_;
    cv_.notify_all();
    lk.unlock();
    drain();                                   // the caller is a worker too
    lk.lock();
    done_.wait(lk, [this]() { return pending_ == 0; });
    jobs_ = nullptr;
  }
  ~CopyPool() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; ++epoch_; }
    cv_.notify_all();
    for (std::thread& t : workers_) t.join();
  }
 private:
  void drain() {
    for (;;) {
      const size_t k = next_.fetch_add(1);
      if (k >= jobs_->size()) return;
      const CopyJob& j = (*jobs_)[k];
      std::memcpy(j.d, j.s, j.n);
    }
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&]() { return epoch_ != seen; });
      seen = epoch_;
      if (stop_) return;
      lk.unlock();
      drain();
      lk.lock();
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::mutex m_; std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  const std::vector<CopyJob>* jobs_ = nullptr;
  std::atomic<size_t> next_{0};
  int pending_ = 0; unsigned long long epoch_ = 0; bool stop_ = false;
};
}  // namespace

static void parallel_copy(const std::vector<std::pair<std::pair<char*, const char*>, size_t>>& pieces, int threads) {
  size_t total = 0;
  for (const auto& p : pieces) total += p.second;
  const size_t chunk = 256 << 10;
  std::vector<CopyJob> jobs;
  for (const auto& p : pieces)
    for (size_t o = 0; o < p.second; o += chunk) jobs.push_back(CopyJob{p.first.first + o, p.first.second + o, std::min(chunk, p.second - o)});
  CopyPool::get().run(jobs, total < (1u << 20) ? 1 : threads);
}

void Frame::computeClosestPointsToNeighbours(std::vector<std::shared_ptr<Frame>>* frames, float thresh) {
  if (fixed) return;  // frame.cpp:93
  Session& S = Session::get();
  S.correspond(*frames, thresh);
  size_t e = 0;
  for (size_t i = 0; i < frames->size(); ++i) {
    Frame& f = *(*frames)[i];
    if (&f != this) { e += f.neighbours.size(); continue; }
    std::vector<std::pair<std::pair<char*, const char*>, size_t>> pieces;
    for (OutgoingEdge& edge : f.neighbours) {
      edge.weight = S.weights[e];
      const size_t n = S.copy_back && S.corr ? (size_t)(S.corr_off[e + 1] - S.corr_off[e]) : 0;
      // frame.cpp:110,158: clear(), then one push_back per kept pair — here the finished slice of the mapped triples (same layout).  A list
      // the vector already holds (same epoch of the library's list, same buffer, same length) is left as it is: after the registration
      // has converged every round reproduces every list, and re-copying cfg4's 198 MB of unchanged triples was 2.3 ms per round
      Session::Held* h = S.copy_back && S.corr && S.epochs && e < S.held.size() ? &S.held[e] : nullptr;
      if (h && h->epoch == S.epochs[e] && h->epoch != 0 && h->n == n && edge.correspondances.size() == n && (const void*)edge.correspondances.data() == h->data) {
        ++S.edges_skipped; ++e; continue;
      }
      edge.correspondances.resize(n);
      if (n) check(mvicp_wait_correspondences(S.ctx, (int)e));   // this edge's chunk has landed (later frames' chunks are still on the bus)
      if (n) pieces.push_back(std::make_pair(std::make_pair((char*)edge.correspondances.data(), (const char*)(S.corr + S.corr_off[e])), n * sizeof(Correspondance)));
      if (h) { h->epoch = S.epochs[e]; h->data = (const void*)edge.correspondances.data(); h->n = n; }
      ++S.edges_copied;
      ++e;
    }
    parallel_copy(pieces, S.copy_threads);
    break;
  }
}

void Frame::recomputeNormals() {
  if (pts.size() < 10) throw std::runtime_error("mvicp: recomputeNormals needs >= 10 points");
  mvicp_ctx* c = nullptr;
  check(mvicp_create(Session::get().device, &c));
  nor.resize(pts.size());
  int st = mvicp_set_num_frames(c, 1);
  if (st == MVICP_OK) st = mvicp_set_frame(c, 0, pts[0].data(), nullptr, (int)pts.size());
  if (st == MVICP_OK) st = mvicp_recompute_normals(c, 0, 10, nor[0].data(), nullptr);
  const std::string err = failure(st);
  mvicp_destroy(c);
  if (st < 0) throw std::runtime_error(err);
  ++version;   // a bound session re-uploads this cloud (new normals) at its next bind
}

// estimateNormals (degree 0) and fitNormals (degree 2 or 3): the call, the fetch into `nor`, the version bump
static std::vector<double> normals_into(Frame* f, int max_nn, double radius, const Vector3d& viewpoint, int degree) {
  std::vector<double> curvature;
  if (f->pts.empty()) { f->nor.clear(); ++f->version; return curvature; }
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(f, &slot);
  const long long n = degree ? mvicp_fit_normals(c, slot, max_nn, radius, viewpoint.data(), degree)
                             : mvicp_estimate_normals(c, slot, max_nn, radius, viewpoint.data());
  if (n < 0) check((int)n);
  std::vector<Vector3d> fresh((size_t)n);
  curvature.assign((size_t)n, 0.0);
  check(mvicp_normals_fetch(c, n, fresh[0].data(), curvature.data(), nullptr));
  f->nor.swap(fresh);
  ++f->version;   // a bound session re-uploads this cloud (new normals) at its next bind
  return curvature;
}

std::vector<double> Frame::estimateNormals(int max_nn, double radius, const Vector3d& viewpoint) { return normals_into(this, max_nn, radius, viewpoint, 0); }

std::vector<double> Frame::fitNormals(int max_nn, double radius, int degree, const Vector3d& viewpoint) {
  if (degree != 2 && degree != 3) throw std::runtime_error("mvicp: fitNormals needs degree 2 or 3");
  return normals_into(this, max_nn, radius, viewpoint, degree);
}

int Frame::orientNormals(int k, double radius) {
  if (pts.empty()) return 0;
  if (nor.size() != pts.size()) throw std::runtime_error("mvicp: orientNormals needs a normal per point");
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot, true);
  const long long comps = mvicp_orient_normals(c, slot, 0, k, radius, MVICP_ORIENT_ANCHOR, nullptr);
  if (comps < 0) check((int)comps);
  std::vector<Vector3d> fresh(pts.size());
  check(mvicp_orient_fetch(c, (long long)fresh.size(), fresh[0].data(), nullptr, nullptr));
  nor.swap(fresh);
  ++version;   // a bound session re-uploads this cloud (new normals) at its next bind
  return (int)comps;
}

int Session::orientFrames(std::vector<std::shared_ptr<Frame>>& frames, float thresh, int min_count, std::vector<unsigned char>* flipped) {
  const int K = (int)frames.size();
  correspond(frames, thresh);
  std::vector<double> P(16 * (size_t)K);
  for (int i = 0; i < K; ++i) std::memcpy(&P[16 * (size_t)i], frames[i]->pose.data(), 128);
  const int E = (int)esrc.size();
  std::vector<int> pos((size_t)E + 1, 0), neg((size_t)E + 1, 0);
  check(mvicp_normal_agreement(ctx, P.data(), pos.data(), neg.data()));
  std::vector<unsigned char> flip((size_t)K, 0);
  const int comps = mvicp_signs_from_agreement(K, E, esrc.data(), edst.data(), pos.data(), neg.data(), min_count, flip.data(), nullptr);
  check(comps);
  for (int i = 0; i < K; ++i) {
    if (!flip[i]) continue;
    Frame& f = *frames[i];
    std::vector<Vector3d> turned(f.nor.size());
    for (size_t j = 0; j < turned.size(); ++j) turned[j] = Vector3d(-f.nor[j][0], -f.nor[j][1], -f.nor[j][2]);
    f.nor.swap(turned);
    ++f.version;
  }
  if (flipped) *flipped = flip;
  return comps;
}

const std::vector<int>& Frame::getNeighbourIndices(size_t num_results) {
  if (pts.empty()) throw std::runtime_error("mvicp: getNeighbours on an empty cloud (nanoflann throws here: nanoflann.hpp:904)");
  if (num_results < 3 || num_results > 16 || num_results > pts.size())
    throw std::runtime_error("mvicp: getNeighbours supports 3 <= num_results <= 16 (and <= the cloud's size); the reference asks for 10 (frame.cpp:249)");
  const unsigned long long generation = Session::get().knn_generation;
  if (knn_k_ == num_results && knn_pts_ == (const void*)pts[0].data() && knn_n_ == pts.size() && knn_version_ == version && knn_generation_ == generation)
    return knn_table_;
  mvicp_ctx* c = nullptr;
  check(mvicp_create(Session::get().device, &c));
  std::vector<int> table(pts.size() * num_results);
  int st = mvicp_set_num_frames(c, 1);
  if (st == MVICP_OK) st = mvicp_set_frame(c, 0, pts[0].data(), nullptr, (int)pts.size());
  if (st == MVICP_OK) st = mvicp_recompute_normals(c, 0, (int)num_results, nullptr, table.data());
  const std::string err = failure(st);
  mvicp_destroy(c);
  if (st < 0) throw std::runtime_error(err);
  knn_table_.swap(table); knn_k_ = num_results; knn_pts_ = (const void*)pts[0].data(); knn_n_ = pts.size();
  knn_version_ = version; knn_generation_ = generation;
  return knn_table_;
}

std::vector<Vector3d> Frame::getNeighbours(int queryIdx, size_t num_results) {
  if (queryIdx < 0 || (size_t)queryIdx >= pts.size()) throw std::runtime_error("mvicp: getNeighbours: queryIdx out of range");
  const std::vector<int>& t = getNeighbourIndices(num_results);
  std::vector<Vector3d> out;
  out.reserve(num_results);
  for (size_t i = 0; i < num_results; ++i) out.push_back(pts[t[(size_t)queryIdx * num_results + i]]);   // frame.cpp:222-226
  return out;
}

mvicp_ctx* Session::query_context(Frame* f, int* slot, bool with_normals) {
  // frame.cpp:187-206.  The reference builds the frame's KD-tree lazily on first use; here the frame's structure already lives in the
  // bound session (uploaded by computeClosestPointsToNeighbours / ceresOptimizer*), found by frame index.  A frame that is not part
  // of the bound vector gets a one-cloud side context owned by the session (built on first use, like the reference's lazy tree;
  // rebuilt when the cloud changes).
  if (f->pts.empty()) throw std::runtime_error("mvicp: getClosestPoint on an empty cloud (nanoflann throws here: nanoflann.hpp:904)");
  const int fi = ctx ? frame_index(f) : -1;
  const bool has_nor = f->nor.size() == f->pts.size();
  if (fi >= 0 && frame_keys[fi].pts == (const void*)f->pts[0].data() && frame_keys[fi].n == f->pts.size() &&
      (!with_normals || (frame_keys[fi].nor == (f->nor.empty() ? nullptr : (const void*)f->nor[0].data()) && frame_keys[fi].version == f->version))) { *slot = fi; return ctx; }
  const bool want_nor = with_normals && has_nor;
  // the same key as the bound path: the frame, its buffers, its size and its version (the normals' buffer only where the side copy holds them)
  const FrameKey key{f, (const void*)f->pts[0].data(), f->pts.size(), f->nor.empty() ? nullptr : (const void*)f->nor[0].data(), f->version};
  const bool same = side_ctx && side_owner == f && side_key.f == f && side_key.pts == key.pts && side_key.n == key.n && side_key.version == key.version &&
                    (!side_nor || side_key.nor == key.nor);
  if (!same || (want_nor && !side_nor)) {
    side_owner = nullptr;   // (forgotten first: a refused upload below leaves a side context nobody owns)
    if (!side_ctx) check(mvicp_create(device, &side_ctx));
    check(mvicp_set_num_frames(side_ctx, 1));
    check(mvicp_set_frame(side_ctx, 0, f->pts[0].data(), want_nor ? f->nor[0].data() : nullptr, (int)f->pts.size()));
    side_owner = f; side_version = f->version; side_nor = want_nor; side_key = key;
  }
  *slot = 0;
  return side_ctx;
}

std::shared_ptr<Frame> Frame::voxelDownsample(double voxel) {
  std::shared_ptr<Frame> out(new Frame());
  out->fixed = fixed; out->pose = pose; out->poseGroundTruth = poseGroundTruth;
  for (const OutgoingEdge& e : neighbours) out->neighbours.push_back(OutgoingEdge{e.neighbourIdx, e.weight, {}});
  if (pts.empty()) return out;
  int slot = 0, has_normals = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot, true);
  const long long m = mvicp_voxel_grid(c, 1, &slot, nullptr, voxel, &has_normals);
  if (m < 0) check((int)m);
  out->pts.assign((size_t)m, Vector3d());
  out->nor.assign(has_normals && nor.size() == pts.size() ? (size_t)m : 0, Vector3d());
  if (m) check(mvicp_voxel_fetch(c, m, out->pts[0].data(), out->nor.empty() ? nullptr : out->nor[0].data(), nullptr));
  return out;
}

std::shared_ptr<Frame> Frame::removeOutliers(int k, double std_ratio, double radius) {
  std::shared_ptr<Frame> out(new Frame());
  out->fixed = fixed; out->pose = pose; out->poseGroundTruth = poseGroundTruth;
  for (const OutgoingEdge& e : neighbours) out->neighbours.push_back(OutgoingEdge{e.neighbourIdx, e.weight, {}});
  if (pts.empty()) return out;
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot, true);
  mvicp_outlier_stats st;
  const long long m = mvicp_outlier_filter(c, slot, k, std_ratio, radius, &st);
  if (m < 0) check((int)m);
  out->pts.assign((size_t)m, Vector3d());
  out->nor.assign(st.has_normals && nor.size() == pts.size() ? (size_t)m : 0, Vector3d());
  if (m) check(mvicp_outlier_fetch(c, m, out->pts[0].data(), out->nor.empty() ? nullptr : out->nor[0].data(), nullptr, 0, nullptr, nullptr));
  return out;
}

std::shared_ptr<Frame> Frame::smoothPoints(int max_nn, double radius, int degree, double max_shift, const Vector3d& viewpoint, std::vector<double>* shift,
                                           std::vector<unsigned char>* moved) {
  std::shared_ptr<Frame> out(new Frame());
  out->fixed = fixed; out->pose = pose; out->poseGroundTruth = poseGroundTruth;
  for (const OutgoingEdge& e : neighbours) out->neighbours.push_back(OutgoingEdge{e.neighbourIdx, e.weight, {}});
  if (shift) shift->clear();
  if (moved) moved->clear();
  if (pts.empty()) return out;
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot);
  const long long n = mvicp_smooth_points(c, slot, max_nn, radius, viewpoint.data(), degree, max_shift);
  if (n < 0) check((int)n);
  out->pts.assign((size_t)n, Vector3d());
  if (shift) shift->assign((size_t)n, 0.0);
  if (moved) moved->assign((size_t)n, 0);
  check(mvicp_smooth_fetch(c, n, out->pts[0].data(), shift ? shift->data() : nullptr, moved ? moved->data() : nullptr, nullptr, nullptr));
  if (nor.size() == pts.size()) {
    out->nor.assign((size_t)n, Vector3d());
    check(mvicp_normals_fetch(c, n, out->nor[0].data(), nullptr, nullptr));
    for (size_t i = 0; i < (size_t)n; ++i) {
      Vector3d& g = out->nor[i];
      if ((g[0] * nor[i][0] + g[1] * nor[i][1]) + g[2] * nor[i][2] < 0.0) g = Vector3d(-g[0], -g[1], -g[2]);
    }
  }
  return out;
}

std::shared_ptr<Frame> Frame::removeSmallClusters(double radius, int min_pts, long long min_size, long long max_clusters, long long* clusters,
                                                  long long* kept_clusters) {
  std::shared_ptr<Frame> out(new Frame());
  out->fixed = fixed; out->pose = pose; out->poseGroundTruth = poseGroundTruth;
  for (const OutgoingEdge& e : neighbours) out->neighbours.push_back(OutgoingEdge{e.neighbourIdx, e.weight, {}});
  if (clusters) *clusters = 0;
  if (kept_clusters) *kept_clusters = 0;
  if (pts.empty()) return out;
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot, true);
  mvicp_cluster_stats st;
  const long long nc = mvicp_cluster(c, slot, radius, min_pts, &st);
  if (nc < 0) check((int)nc);
  const long long m = mvicp_cluster_select(c, min_size, max_clusters);
  if (m < 0) check((int)m);
  out->pts.assign((size_t)m, Vector3d());
  out->nor.assign(st.has_normals && nor.size() == pts.size() ? (size_t)m : 0, Vector3d());
  if (m) check(mvicp_cluster_fetch_kept(c, m, out->pts[0].data(), out->nor.empty() ? nullptr : out->nor[0].data(), nullptr, nullptr));
  if (clusters) *clusters = nc;
  if (kept_clusters && nc) {
    std::vector<int> size((size_t)nc);
    std::vector<unsigned char> keep((size_t)nc);
    check(mvicp_cluster_fetch(c, 0, nullptr, nullptr, nc, size.data()));
    check(mvicp_cluster_keep_rule(nc, size.data(), min_size, max_clusters, keep.data()));
    for (unsigned char k : keep) *kept_clusters += k;
  }
  return out;
}

std::shared_ptr<Frame> Frame::removePlane(double tau, long long hypotheses, unsigned long long seed, const double* axis, double cos_min, bool keep_plane,
                                          mvicp_plane_result* result) {
  std::shared_ptr<Frame> out(new Frame());
  out->fixed = fixed; out->pose = pose; out->poseGroundTruth = poseGroundTruth;
  for (const OutgoingEdge& e : neighbours) out->neighbours.push_back(OutgoingEdge{e.neighbourIdx, e.weight, {}});
  mvicp_plane_result R;
  std::memset(&R, 0, sizeof(R));
  R.best = -1;
  if (result) *result = R;
  if (pts.empty()) return out;
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot, true);
  check(mvicp_segment_plane(c, slot, hypotheses, seed, tau, axis, cos_min, 1, &R));
  const long long m = mvicp_plane_select(c, keep_plane ? 1 : 0);
  if (m < 0) check((int)m);
  out->pts.assign((size_t)m, Vector3d());
  out->nor.assign(R.has_normals && nor.size() == pts.size() ? (size_t)m : 0, Vector3d());
  if (m) check(mvicp_plane_fetch_kept(c, m, out->pts[0].data(), out->nor.empty() ? nullptr : out->nor[0].data(), nullptr));
  if (result) *result = R;
  return out;
}

std::vector<unsigned char> Frame::boundaryPoints(int max_nn, double radius, double cos_gap) {
  std::vector<unsigned char> flag;
  if (pts.empty()) return flag;
  if (nor.size() != pts.size()) throw std::runtime_error("mvicp: boundaryPoints needs normals");
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot, true);
  const long long flagged = mvicp_boundary(c, slot, 0, max_nn, radius, cos_gap);
  if (flagged < 0) check((int)flagged);
  flag.assign(pts.size(), 0);
  check(mvicp_boundary_fetch(c, (long long)flag.size(), flag.data(), nullptr, nullptr, nullptr));
  return flag;
}

std::vector<int> Frame::issKeypoints(double salient_radius, double non_max_radius, double gamma21, double gamma32, int min_neighbors) {
  std::vector<int> idx;
  if (pts.empty()) return idx;
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot);
  const long long k = mvicp_iss_keypoints(c, slot, salient_radius, non_max_radius, gamma21, gamma32, min_neighbors);
  if (k < 0) check((int)k);
  idx.assign((size_t)k, 0);
  if (k) check(mvicp_iss_fetch(c, k, idx.data(), nullptr, nullptr, 0, nullptr, nullptr, nullptr));
  return idx;
}

double Frame::getClosestPoint(const Vector3d& q, size_t& ret_index) {
  int slot = 0, idx = -1;
  double d2 = 0.0;
  mvicp_ctx* c = Session::get().query_context(this, &slot);
  check(mvicp_nn_query(c, slot, q.data(), 1, MVICP_NN_AUTO, &idx, &d2));
  ret_index = (size_t)idx;
  return d2;
}

std::vector<double> Frame::getClosestPoints(const std::vector<Vector3d>& q, std::vector<size_t>& ret_index) {
  int slot = 0;
  mvicp_ctx* c = Session::get().query_context(this, &slot);
  const int n = (int)q.size();
  std::vector<double> d2(q.size());
  std::vector<int> idx(q.size());
  ret_index.resize(q.size());
  if (n == 0) return d2;
  check(mvicp_nn_query(c, slot, q[0].data(), n, MVICP_NN_AUTO, idx.data(), d2.data()));
  for (int i = 0; i < n; ++i) ret_index[i] = (size_t)idx[i];
  return d2;
}

}  // namespace mvicp

namespace ICP_Ceres {

void ceresOptimizer(std::vector<std::shared_ptr<Frame>>& frames, bool pointToPlane, bool robust) {
  mvicp::Session::get().optimize(frames, MVICP_PARAM_EIGEN_QUATERNION, pointToPlane, robust);
}
void ceresOptimizer_ceresAngleAxis(std::vector<std::shared_ptr<Frame>>& frames, bool pointToPlane, bool robust) {
  mvicp::Session::get().optimize(frames, MVICP_PARAM_ANGLE_AXIS, pointToPlane, robust);
}
void ceresOptimizer_sophusSE3(std::vector<std::shared_ptr<Frame>>& frames, bool pointToPlane, bool robust, bool) {
  mvicp::Session::get().optimize(frames, MVICP_PARAM_SOPHUS_SE3, pointToPlane, robust);
}

// icp-ceres.cpp:137-218,525-565: one residual block per index-aligned pair (dst[i], src[i]), single free pose from identity,
// no loss function.  Frame 0 = dst (fixed, identity), frame 1 = src.
static Isometry3d pairwise(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, std::vector<Vector3d>* nor, int param) {
  auto check = [](int st) { if (st < 0) throw std::runtime_error(std::string("mvicp: ") + mvicp_last_error()); };
  if (src.size() != dst.size() || src.empty()) throw std::runtime_error("mvicp: pairwise needs equally sized, non-empty clouds");
  mvicp_ctx* c = nullptr;
  check(mvicp_create(mvicp::Session::get().device, &c));
  check(mvicp_set_num_frames(c, 2));
  check(mvicp_set_frame(c, 0, dst[0].data(), nor ? (*nor)[0].data() : nullptr, (int)dst.size()));
  check(mvicp_set_frame(c, 1, src[0].data(), nullptr, (int)src.size()));
  const int s = 1, d = 0;
  check(mvicp_set_graph(c, 1, &s, &d));
  std::vector<int> id(src.size());
  std::iota(id.begin(), id.end(), 0);
  check(mvicp_set_correspondences(c, 0, (int)id.size(), id.data(), id.data(), 0.f));
  double P[32];
  Isometry3d I;
  std::memcpy(P, I.data(), 128);
  std::memcpy(P + 16, I.data(), 128);
  unsigned char fixed[2] = {1, 0};
  mvicp_summary sm;
  const int st = mvicp_optimize(c, P, fixed, param, nor != nullptr, 0, 50, &sm);
  Isometry3d out;
  std::memcpy(out.data(), P + 16, 128);
  mvicp_destroy(c);
  check(st);
  return out;
}
Isometry3d pointToPoint_EigenQuaternion(std::vector<Vector3d>& s, std::vector<Vector3d>& d) { return pairwise(s, d, nullptr, MVICP_PARAM_EIGEN_QUATERNION); }
Isometry3d pointToPoint_CeresAngleAxis(std::vector<Vector3d>& s, std::vector<Vector3d>& d) { return pairwise(s, d, nullptr, MVICP_PARAM_ANGLE_AXIS); }
Isometry3d pointToPoint_SophusSE3(std::vector<Vector3d>& s, std::vector<Vector3d>& d, bool) { return pairwise(s, d, nullptr, MVICP_PARAM_SOPHUS_SE3); }
Isometry3d pointToPlane_EigenQuaternion(std::vector<Vector3d>& s, std::vector<Vector3d>& d, std::vector<Vector3d>& n) { return pairwise(s, d, &n, MVICP_PARAM_EIGEN_QUATERNION); }
Isometry3d pointToPlane_CeresAngleAxis(std::vector<Vector3d>& s, std::vector<Vector3d>& d, std::vector<Vector3d>& n) { return pairwise(s, d, &n, MVICP_PARAM_ANGLE_AXIS); }
Isometry3d pointToPlane_SophusSE3(std::vector<Vector3d>& s, std::vector<Vector3d>& d, std::vector<Vector3d>& n, bool) { return pairwise(s, d, &n, MVICP_PARAM_SOPHUS_SE3); }

}  // namespace ICP_Ceres

namespace ICP_Closedform {
static void check(int st) { if (st < 0) throw std::runtime_error(std::string("mvicp: ") + mvicp_last_error()); }
Isometry3d pointToPoint(std::vector<Vector3d>& src, std::vector<Vector3d>& dst) {
  if (src.size() != dst.size() || src.empty()) throw std::runtime_error("mvicp: closed form needs equally sized, non-empty clouds");
  Isometry3d T;
  check(mvicp_closedform_point_to_point(src[0].data(), dst[0].data(), (int)src.size(), T.data()));
  return T;
}
Isometry3d pointToPlane(std::vector<Vector3d>& src, std::vector<Vector3d>& dst, std::vector<Vector3d>& nor) {
  if (src.size() != dst.size() || src.size() != nor.size() || src.empty()) throw std::runtime_error("mvicp: closed form needs equally sized, non-empty clouds");
  Isometry3d T;
  check(mvicp_closedform_point_to_plane(src[0].data(), dst[0].data(), nor[0].data(), (int)src.size(), T.data()));
  return T;
}
}  // namespace ICP_Closedform
