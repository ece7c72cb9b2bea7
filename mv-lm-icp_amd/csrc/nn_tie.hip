// Tie fix-up of the 1-NN kernels: the reference's own exact search, on the reference's own tree, for the (rare) queries whose best
// distance is met by more than one target.  See nn_tie.h.
//
// The walk itself is tie_walk.h (nanoflann's findNeighbors / searchLevel for a result set of capacity 1, over kdvisit.h's restatement of the
// split structure buildIndex produces with leaf_max_size = 1, frame.cpp:189 — the one normals.hip already uses for the k-NN tie order); this TU is
// built with -ffp-contract=off, as that header demands.
//
// The walk's stack holds one pending subtree per level of the tree.  A target whose tree has at most TIE_STACK levels (every ordinary cloud: a random
// cloud of 200 000 points has 22) is answered by nn_tie_kernel from a per-lane array; a deeper one (coordinates in geometric progression make a tree as
// deep as it has points) by nn_tie_deep_kernel, the same loop over the same list with each lane's stack in global memory, sized from the levels
// build_visit_tree reported.  Each kernel skips the other's jobs; the deep one is launched only when a job of the launch has such a target.
#include <algorithm>
#include <thread>

#include "kdvisit.h"
#include "nn_metric.h"
#include "nn_tie.h"
#include "tie_walk.h"

namespace mvicp {

namespace {

constexpr int TIE_STACK = 128;   // pending subtrees of nn_tie_kernel: one per level of the tree; a balanced tree of 2^30 points has 31 levels, skewed clouds more
                                 // (40 B each, in scratch memory: 5 KB per lane of this small kernel only)
constexpr int TIE_DEEP_LANES = 1024;        // lanes of nn_tie_deep_kernel (16 blocks of 64): each owns `levels` entries of the context's global stack
constexpr int TIE_MAX_LEVELS = 16384;       // deeper trees are refused by ensure_tie_trees (include/mvicp.h): 1024 lanes x 16384 x 40 B = 640 MB would be the stack

// One pass over the reported queries.  DEEP = false: the jobs whose tree fits the per-lane array; DEEP = true: the others, on `deep_st` (deep_cap entries
// per lane of the grid).
template <bool DEEP>
__device__ __forceinline__ void tie_pass(const TieJob* __restrict__ jobs, int n_jobs, const unsigned long long* __restrict__ list, unsigned int reported,
                                         unsigned int cap, double bound, unsigned int* __restrict__ seen, TiePending* __restrict__ st, int st_cap) {
  const bool everything = reported > cap;                       // the list overflowed: re-answer every query of the launch
  const long long total = everything ? jobs[n_jobs - 1].q_begin + jobs[n_jobs - 1].n : (long long)reported;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    int jb, i;
    if (everything) {
      int lo = 0, hi = n_jobs - 1;
      while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].q_begin <= t) lo = mid; else hi = mid - 1; }
      jb = lo; i = (int)(t - jobs[lo].q_begin);
    } else {
      const unsigned long long e = list[t];
      jb = (int)(e >> 32); i = (int)(e & 0xffffffffull);
    }
    const TieJob& J = jobs[jb];
    if (i >= J.n) continue;
    if (J.nodes == nullptr) { if (!DEEP) seen[1] = 1u; continue; }   // lazy trees (api.cpp): this target has none yet — the host builds it and repeats the search
    if ((J.levels > TIE_STACK) != DEEP) continue;                    // the other kernel's job
    const int cur = J.out_idx[i];
    if (cur < 0) continue;
    double qx, qy, qz;
    {
      const double p0 = J.q[3 * (size_t)i], p1 = J.q[3 * (size_t)i + 1], p2 = J.q[3 * (size_t)i + 2];
      if (J.xf != nullptr) xf_point(J.xf, p0, p1, p2, qx, qy, qz);   // the same rounded operations as the search kernels
      else { qx = p0; qy = p1; qz = p2; }
    }
    double d2 = 0.0;
    const TieTree T{static_cast<const VisitNode*>(J.nodes), J.ord, J.tpts, J.box};
    const int bi = tie_walk(T, qx, qy, qz, st, st_cap, &d2);
    if (bi == TIE_WALK_TRUNCATED) { seen[2] = 1u; continue; }   // (cannot happen: the stack has the tree's levels; the host turns it into an error status)
    if (bi < 0 || d2 != J.out_d2[i]) continue;   // (cannot happen: both are the exact minimum)
    const int pos = J.inv ? J.inv[bi] : bi;
    if (pos != cur) {
      J.out_idx[i] = pos;
      if (J.list.dirty) update_list_entry(J.list, i, pos, d2, bound, false);
    }
  }
}

__global__ __launch_bounds__(64) void nn_tie_kernel(const TieJob* __restrict__ jobs, int n_jobs, const unsigned long long* __restrict__ list,
                                                    const unsigned int* __restrict__ count, unsigned int* __restrict__ next_count, unsigned int cap,
                                                    double bound, unsigned int* __restrict__ seen) {
  const unsigned int reported = *count;
  if (blockIdx.x == 0 && threadIdx.x == 0) { *next_count = 0u; *seen = reported; }   // two counters alternate between launches (like the grid kernel's far list)
  if (reported == 0u) return;
  TiePending st[TIE_STACK];
  tie_pass<false>(jobs, n_jobs, list, reported, cap, bound, seen, st, TIE_STACK);
}

// the targets with more than TIE_STACK levels: launched right behind nn_tie_kernel on the same stream, reads the same counter (that kernel only zeroes
// the OTHER one) and the same list
__global__ __launch_bounds__(64) void nn_tie_deep_kernel(const TieJob* __restrict__ jobs, int n_jobs, const unsigned long long* __restrict__ list,
                                                         const unsigned int* __restrict__ count, unsigned int cap, double bound,
                                                         unsigned int* __restrict__ seen, TiePending* __restrict__ deep_st, int deep_cap) {
  const unsigned int reported = *count;
  if (reported == 0u) return;
  TiePending* st = deep_st + (size_t)(blockIdx.x * blockDim.x + threadIdx.x) * (size_t)deep_cap;
  tie_pass<true>(jobs, n_jobs, list, reported, cap, bound, seen, st, deep_cap);
}

}  // namespace

// ---- host ----------------------------------------------------------------------------------------------------------------------------
void free_tie(FrameDev& f) {
  if (f.tie_nodes) (void)hipFree(f.tie_nodes);
  if (f.tie_ord) (void)hipFree(f.tie_ord);
  if (f.tie_slot) (void)hipFree(f.tie_slot);
  f.tie_nodes = nullptr; f.tie_ord = nullptr; f.tie_slot = nullptr; f.has_tie = false; f.tie_levels = 0;
}

int ensure_tie_trees(mvicp_ctx* c, const std::vector<int>& frames) {
  std::vector<int> todo;
  for (int f : frames)
    if (f >= 0 && f < c->n_frames && !c->frames[f].has_tie && c->frames[f].n > 0 && std::find(todo.begin(), todo.end(), f) == todo.end()) todo.push_back(f);
  if (todo.empty()) return MVICP_OK;
  struct Built { std::vector<double> xyz; std::vector<VisitNode> nodes; std::vector<int> slot, ord; double box[6]; int levels; };
  std::vector<Built> B(todo.size());
  for (size_t k = 0; k < todo.size(); ++k) {
    const FrameDev& F = c->frames[todo[k]];
    B[k].xyz.resize(3 * (size_t)F.n);
    MV_HIP(hipMemcpy(B[k].xyz.data(), F.pts, sizeof(double) * 3 * (size_t)F.n, hipMemcpyDeviceToHost));
  }
  // the trees are independent: build them side by side (0.07 s per 200 k points, 0.5 s per 1 M on one core)
  auto work = [&](size_t k) {
    Built& b = B[k];
    const int n = (int)(b.xyz.size() / 3);
    b.levels = build_visit_tree(b.xyz.data(), n, b.nodes, b.slot);
    b.ord.assign(n, 0);
    for (int i = 0; i < n; ++i) b.ord[b.slot[i]] = i;
    for (int a = 0; a < 3; ++a) b.box[a] = b.box[3 + a] = b.xyz[a];
    for (int i = 1; i < n; ++i)
      for (int a = 0; a < 3; ++a) { const double v = b.xyz[3 * (size_t)i + a]; if (v < b.box[a]) b.box[a] = v; if (v > b.box[3 + a]) b.box[3 + a] = v; }
  };
  const unsigned int nthreads = std::max(1u, std::min<unsigned int>({(unsigned int)todo.size(), std::thread::hardware_concurrency(), 16u}));
  if (nthreads <= 1) { for (size_t k = 0; k < todo.size(); ++k) work(k); }
  else {
    std::vector<std::thread> pool;
    for (unsigned int t = 0; t < nthreads; ++t) pool.emplace_back([&, t]() { for (size_t k = t; k < todo.size(); k += nthreads) work(k); });
    for (auto& th : pool) th.join();
  }
  // the fix-up's walk holds one pending subtree per level: a tree it could not walk to the end is refused here, not answered from
  for (size_t k = 0; k < todo.size(); ++k)
    if (B[k].levels > TIE_MAX_LEVELS) {
      set_error("frame %d: its nanoflann-equivalent tree has %d levels, the tie fix-up walks at most %d (tie_rule = 0 searches such a cloud with the lowest-index rule)",
                todo[k], B[k].levels, TIE_MAX_LEVELS);
      return MVICP_ERR_ARG;
    }
  for (size_t k = 0; k < todo.size(); ++k) {
    FrameDev& F = c->frames[todo[k]];
    auto upload = [&]() -> int {
      MV_HIP(hipMalloc(&F.tie_nodes, sizeof(VisitNode) * B[k].nodes.size()));
      MV_HIP(hipMemcpy(F.tie_nodes, B[k].nodes.data(), sizeof(VisitNode) * B[k].nodes.size(), hipMemcpyHostToDevice));
      MV_HIP(hipMalloc((void**)&F.tie_ord, sizeof(int) * B[k].ord.size()));
      MV_HIP(hipMemcpy(F.tie_ord, B[k].ord.data(), sizeof(int) * B[k].ord.size(), hipMemcpyHostToDevice));
      MV_HIP(hipMalloc((void**)&F.tie_slot, sizeof(int) * B[k].slot.size()));
      MV_HIP(hipMemcpy(F.tie_slot, B[k].slot.data(), sizeof(int) * B[k].slot.size(), hipMemcpyHostToDevice));
      return MVICP_OK;
    };
    const int st = upload();
    if (st != MVICP_OK) { free_tie(F); return st; }   // a half-uploaded tree is released, not leaked at the next attempt
    for (int a = 0; a < 6; ++a) F.tie_box[a] = B[k].box[a];
    F.tie_levels = B[k].levels;
    F.has_tie = true;
  }
  return MVICP_OK;
}

TieRef tie_ref(mvicp_ctx* c, size_t launch_queries, unsigned int job) {
  TieRef T{nullptr, nullptr, 0u, job};
  if (!c->opt.tie_rule) return T;
  // capacity: every query of the launch up to 4 M entries (32 MB); beyond that an overflow makes the fix-up re-answer the whole launch
  const size_t want = std::min<size_t>(std::max<size_t>(launch_queries, 1024), (size_t)4 << 20);
  if (want > c->tie_cap) {
    if (c->d_tie_list) { if (hipStreamSynchronize(c->stream) != hipSuccess || hipFree(c->d_tie_list) != hipSuccess) return T; c->d_tie_list = nullptr; c->tie_cap = 0; }
    if (hipMalloc((void**)&c->d_tie_list, sizeof(unsigned long long) * want) != hipSuccess) return T;
    c->tie_cap = want;
  }
  if (!c->d_tie_count) {
    if (hipMalloc((void**)&c->d_tie_count, 2 * sizeof(unsigned int)) != hipSuccess) return T;
    if (hipMemset(c->d_tie_count, 0, 2 * sizeof(unsigned int)) != hipSuccess) return T;
    c->tie_parity = 0;
  }
  T.list = c->d_tie_list; T.count = c->d_tie_count + c->tie_parity; T.cap = (unsigned int)c->tie_cap;
  return T;
}

void tie_job_fill(const FrameDev& F, TieJob& j) {
  j.nodes = F.has_tie ? F.tie_nodes : nullptr; j.ord = F.tie_ord; j.tpts = F.pts;
  for (int a = 0; a < 6; ++a) j.box[a] = F.tie_box[a];
  j.levels = F.has_tie ? F.tie_levels : 0;
}

int launch_tie_fixup(mvicp_ctx* c, const std::vector<TieJob>& jobs, double d2_bound) {
  if (!c->opt.tie_rule || jobs.empty() || !c->d_tie_count) return MVICP_OK;
  if (!c->h_tie_seen) {
    MV_HIP(hipHostMalloc((void**)&c->h_tie_seen, 4 * sizeof(unsigned int), hipHostMallocMapped));   // [0] reports of the launch, [1] "a reported query's target has no tree", [2] "a walk ran out of stack"
    c->h_tie_seen[0] = 1u;   // unknown until a launch has written it
    c->h_tie_seen[1] = 0u; c->h_tie_seen[2] = 0u; c->h_tie_seen[3] = 0u;
    MV_HIP(hipHostGetDevicePointer((void**)&c->d_tie_seen, c->h_tie_seen, 0));
  }
  std::vector<TieJob> tab(jobs);
  long long off = 0;
  for (TieJob& j : tab) { j.q_begin = off; off += j.n; }
  TieJob* d_tab = nullptr;
  MV_CHECK(cached_upload(c, "tie_jobs", tab.data(), sizeof(TieJob) * tab.size(), (void**)&d_tab));
  unsigned int* cnt = c->d_tie_count + c->tie_parity;
  unsigned int* nxt = c->d_tie_count + (c->tie_parity ^ 1);
  c->tie_parity ^= 1;
  c->h_tie_seen[1] = 0u;   // (host store to the mapped word before the launch; the kernel only ever stores 1)
  c->h_tie_seen[2] = 0u;
  int deep_levels = 0;     // the deepest target of this launch that nn_tie_kernel's per-lane array cannot hold
  for (const TieJob& j : tab) if (j.nodes != nullptr && j.levels > TIE_STACK) deep_levels = std::max(deep_levels, j.levels);
  if (deep_levels > 0) {
    const size_t want = (size_t)TIE_DEEP_LANES * (size_t)deep_levels * sizeof(TiePending);
    if (want > c->tie_deep_bytes) {
      if (c->d_tie_deep) { MV_HIP(hipStreamSynchronize(c->stream)); MV_HIP(hipFree(c->d_tie_deep)); c->d_tie_deep = nullptr; c->tie_deep_bytes = 0; }
      MV_HIP(hipMalloc(&c->d_tie_deep, want));
      c->tie_deep_bytes = want;
    }
  }
  ProfScope ps(c, "nn_tie", 0.0);
  hipLaunchKernelGGL(nn_tie_kernel, dim3(256), dim3(64), 0, c->stream, d_tab, (int)tab.size(), c->d_tie_list, cnt, nxt, (unsigned int)c->tie_cap, d2_bound, c->d_tie_seen);
  MV_HIP(hipGetLastError());
  if (deep_levels > 0) {
    hipLaunchKernelGGL(nn_tie_deep_kernel, dim3(TIE_DEEP_LANES / 64), dim3(64), 0, c->stream, d_tab, (int)tab.size(), c->d_tie_list, cnt, (unsigned int)c->tie_cap, d2_bound,
                       c->d_tie_seen, static_cast<TiePending*>(c->d_tie_deep), deep_levels);
    MV_HIP(hipGetLastError());
  }
  return MVICP_OK;
}

}  // namespace mvicp
