// DBSCAN / Euclidean cluster extraction over one stored cloud (mvicp_cluster, mvicp_cluster_select): which points belong together.  The
// result is a pure function of the stored cloud, bit for bit (the contract is stated in include/mvicp.h; tests/clusterref.py is its numpy
// form).  Only comparisons and integers enter: the predicate dist2 < B2 of the radius searches, counts, connected components and a minimum
// over the strict total order (dist2, original index).  DESIGN.md §3.18.
//
// Passes of mvicp_cluster, all on the context's stream, one host wait at the end:
//   1  core     one lane per point in hash-CELL order (GridDev::crec): traverse() of knn_traverse.h without a box tree, counting the
//               candidates with d2 < B2 and stopping once the scanned block's faces lie B2 away or the count has reached min_pts.
//               Writes the core byte and parent[i] = i in original order.
//   2  union    one lane per CORE point, the same traversal to the radius: every core j < i with d2 < B2 is united with i in the parent
//               array.  find halves the path; the larger root is hooked onto the smaller by atomicCAS and the loser of a race goes on
//               from the value the CAS returned.  A parent only ever decreases, so no cycle can form, every retry starts strictly lower
//               (some lane always progresses, nobody waits for a value another lane has yet to write), and a component's root ends as
//               its smallest index -- the contract's anchor -- whatever order the lanes ran in.
//      roots    after the kernel boundary: root[i] = the end of i's parent chain, flag[i] = (i is its own root), core points only
//   3  border   one lane per NON-core point: the minimum of (d2, j) over the core candidates with d2 < B2 in a register pair;
//               root[i] = root[that j], or -1 (noise).  A minimum over a strict total order: the visiting order cannot matter.
//   4  label    exclusive scan of the root flags over the original index (rocprim) = the rank of a root among the roots = the contract's
//               numbering; label[i] = rank[root[i]]; sizes and the three counts by integer atomics, one per distinct label of a wave.
// mvicp_cluster_select: keep byte per cluster from the host rule (mvicp_cluster_keep_rule), flag = label >= 0 and kept, then select_rows
// (row_select.h) with the label as a fourth row.
// The radius graph is undirected because dist2 is bitwise symmetric (the differences are exact negatives, the squares drop the sign), so
// "j < i" in the union pass loses no edge.  Every store is a plain vector store or a vector atomic; no kernel waits for another workgroup.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "knn_traverse.h"
#include "nn_metric.h"
#include "row_select.h"

namespace mvicp {

namespace {

constexpr int NT = 128;   // lanes per workgroup of the traversal kernels
constexpr int VT = 256;   // of the streaming passes

struct ClCtl { int clusters, core, border, noise; };

struct ClJob {
  GridView g;
  double B2; int min_pts;
  unsigned char* core;   // n, original order
  int* parent;           // n: the union-find forest over the core points
  int* root;             // n: the cluster's smallest core index, -1 for noise
};

__device__ __forceinline__ int ld_parent(const int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(NT) void cluster_core_kernel(ClJob job) {
  const int i = blockIdx.x * NT + threadIdx.x;   // position in cell order
  if (i >= job.g.n) return;
  const PointRec me = job.g.crec[i];
  const double B2 = job.B2;
  const int need = job.min_pts;
  int cnt = 0;
  auto offer = [&](double d, const PointRec*) { cnt += d < B2 ? 1 : 0; };
  auto reset = [&]() { cnt = 0; };
  auto stop = [&](double m2) { return m2 >= B2 || cnt >= need; };
  auto open = [](double) { return true; };
  auto seed = [](double) {};
  traverse(job.g, nullptr, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);
  job.core[me.idx] = cnt >= need ? 1 : 0;
  job.parent[me.idx] = (int)me.idx;
}

// the root of x's chain, halving the path on the way.  Every value ever stored in parent[x] is x or an ancestor of x below it, so a
// stale read or a halving store that lands late only lengthens a walk
__device__ __forceinline__ int find_root(int* parent, int x) {
  for (;;) {
    const int p = ld_parent(parent, x);
    if (p == x) return x;
    const int gp = ld_parent(parent, p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
}

// unites the trees of a and b -> the root of the united tree at that moment (later an ancestor-or-self of both)
__device__ __forceinline__ int unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a); b = find_root(parent, b);
    if (a == b) return a;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = old; b = lo;   // hi was hooked by someone else meanwhile: old < hi, the pair to unite is now (old, lo)
  }
}

__global__ __launch_bounds__(NT) void cluster_union_kernel(ClJob job) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= job.g.n) return;
  const PointRec me = job.g.crec[i];
  const int mi = (int)me.idx;
  if (!job.core[mi]) return;
  const double B2 = job.B2;
  int up = mi;   // the lane's way into its tree: mi or an ancestor of it, the root as of the last union (one load finds out whether it still is)
  auto offer = [&](double d, const PointRec* p) {
    const int j = (int)p->idx;
    if (d < B2 && j < mi && job.core[j] && ld_parent(job.parent, j) != up) up = unite(job.parent, up, j);   // (parent[j] == up: already one tree)
  };
  auto reset = []() {};   // (uniting a pair again changes nothing)
  auto stop = [&](double m2) { return m2 >= B2; };
  auto open = [](double) { return true; };
  auto seed = [](double) {};
  traverse(job.g, nullptr, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);
}

__global__ __launch_bounds__(VT) void cluster_root_kernel(const unsigned char* __restrict__ core, const int* __restrict__ parent, int n, int* __restrict__ root,
                                                          int* __restrict__ flag) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  int f = 0;
  if (core[i]) {
    int r = i;
    for (int p = parent[r]; p != r; p = parent[r]) r = p;   // (r decreases: the walk ends)
    root[i] = r;
    f = r == i ? 1 : 0;
  }
  flag[i] = f;
}

__global__ __launch_bounds__(NT) void cluster_border_kernel(ClJob job) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= job.g.n) return;
  const PointRec me = job.g.crec[i];
  const int mi = (int)me.idx;
  if (job.core[mi]) return;
  const double B2 = job.B2;
  double bd = INFINITY; int bj = -1;
  auto offer = [&](double d, const PointRec* p) {
    const int j = (int)p->idx;
    if (d < B2 && (d < bd || (d == bd && j < bj)) && job.core[j]) { bd = d; bj = j; }   // (d < B2 < +inf = the first bd: bj = -1 never meets d == bd)
  };
  auto reset = []() {};   // (a minimum: offering a point again changes nothing)
  auto stop = [&](double m2) { return m2 >= B2; };
  auto open = [](double) { return true; };
  auto seed = [](double) {};
  traverse(job.g, nullptr, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);
  job.root[mi] = bj >= 0 ? job.root[bj] : -1;   // (root of a core point: written by the kernel before this one)
}

// one atomic per distinct value of `key` among the wave's lanes with on set: the lowest such lane adds the number of its equals
__device__ __forceinline__ void wave_count(bool on, int key, int* base) {
  unsigned long long left = __ballot(on);
  while (left) {
    const int leader = __ffsll((long long)left) - 1;
    const int k = __shfl(key, leader, 64);
    const unsigned long long eq = __ballot(on && key == k) & left;
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(base + k, (int)__popcll(eq));
    left &= ~eq;
  }
}

__global__ __launch_bounds__(VT) void cluster_label_kernel(const unsigned char* __restrict__ core, const int* __restrict__ root, const int* __restrict__ flag,
                                                           const int* __restrict__ pos, int n, int* __restrict__ label, int* __restrict__ size,
                                                           ClCtl* __restrict__ ctl) {
  const int i = blockIdx.x * VT + threadIdx.x;
  const bool in = i < n;
  int lab = -1, kind = 2;   // kind: 0 core, 1 border, 2 noise
  if (in) {
    const int r = root[i];
    if (r >= 0) lab = pos[r];
    kind = core[i] ? 0 : lab >= 0 ? 1 : 2;
    label[i] = lab;
    if (i == n - 1) ctl->clusters = pos[i] + flag[i];
  }
  wave_count(in && lab >= 0, lab, size);
  wave_count(in, kind, &ctl->core);   // core, border, noise are consecutive ints
}

__global__ __launch_bounds__(VT) void cluster_keep_kernel(const int* __restrict__ label, const unsigned char* __restrict__ keep, int n, int* __restrict__ flag) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  const int lab = label[i];
  flag[i] = lab >= 0 && keep[lab] ? 1 : 0;
}

// the arena of a frame of n points: [control | core | parent | root | root flag | root rank | label | size | keep]
struct Arena {
  size_t core, parent, root, flag, pos, label, size, keep, bytes;
  explicit Arena(size_t n) {
    size_t o = 256;
    auto take = [&](size_t b) { const size_t at = o; o += align256(std::max<size_t>(b, 1)); return at; };
    core = take(n); parent = take(4 * n); root = take(4 * n); flag = take(4 * n); pos = take(4 * n); label = take(4 * n); size = take(4 * n); keep = take(n);
    bytes = o;
  }
};

}  // namespace

long long cluster_points(mvicp_ctx* c, const FrameDev& f, int frame, double B2, int min_pts, mvicp_cluster_stats* stats) {
  ClusterStage& S = c->clu;
  S.drop_result();   // (the last result ends here; a failed call leaves none behind)
  mvicp_cluster_stats R;
  std::memset(&R, 0, sizeof(R));
  R.n = f.n; R.has_normals = f.nor ? 1 : 0; R.largest_label = -1;
  if (f.n == 0) { S.n = 0; S.clusters = 0; S.frame = frame; if (stats) *stats = R; return 0; }
  if (!f.has_grid) { set_error("clustering needs the per-cloud hash structure"); return MVICP_ERR_STATE; }
  {
    // no dist2 of this cloud can overflow: |d_a| <= 2 a per axis, and every operation of dist2 is monotone in |d_a|
    const double t = f.grid.maxabs + f.grid.maxabs;
    if (!std::isfinite((t * t + t * t) + t * t)) { set_error("cluster: a neighbour distance can overflow (largest |coordinate| %g)", f.grid.maxabs); return MVICP_ERR_ARG; }
  }
  const int n = f.n;
  const size_t NN = (size_t)n;
  hipStream_t st = c->stream;

  const Arena A(NN);
  MV_CHECK(S.dev.reserve(A.bytes));
  MV_CHECK(S.pin.reserve(256 + align256(4 * NN)));   // [control | size, later the keep bytes]
  MV_CHECK(S.sel.reserve(n, true, st));
  char* D = S.dev.p;
  ClCtl* d_ctl = reinterpret_cast<ClCtl*>(D);
  ClCtl* h_ctl = reinterpret_cast<ClCtl*>(S.pin.p);
  int* parent = reinterpret_cast<int*>(D + A.parent); int* root = reinterpret_cast<int*>(D + A.root);
  int* flag = reinterpret_cast<int*>(D + A.flag); int* pos = reinterpret_cast<int*>(D + A.pos);
  S.core = reinterpret_cast<unsigned char*>(D + A.core); S.label = reinterpret_cast<int*>(D + A.label); S.size = reinterpret_cast<int*>(D + A.size);
  S.keep = reinterpret_cast<unsigned char*>(D + A.keep);
  size_t scan_bytes = 0;
  MV_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag, pos, 0, NN, rocprim::plus<int>(), st));
  MV_CHECK(S.tmp.reserve(std::max<size_t>(scan_bytes, 256)));

  MV_HIP(hipMemsetAsync(d_ctl, 0, sizeof(ClCtl), st));
  MV_HIP(hipMemsetAsync(S.size, 0, 4 * NN, st));
  ClJob j;
  fill_grid_view(&j.g, f.grid, n);
  j.B2 = B2; j.min_pts = min_pts; j.core = S.core; j.parent = parent; j.root = root;
  {
    ProfScope ps(c, "cluster_core", 0.0);
    hipLaunchKernelGGL(cluster_core_kernel, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
  }
  MV_HIP(hipGetLastError());
  {
    ProfScope ps(c, "cluster_union", 0.0);
    hipLaunchKernelGGL(cluster_union_kernel, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
    hipLaunchKernelGGL(cluster_root_kernel, dim3(grid_of(n, VT)), dim3(VT), 0, st, S.core, parent, n, root, flag);
  }
  MV_HIP(hipGetLastError());
  {
    ProfScope ps(c, "cluster_border", 0.0);
    hipLaunchKernelGGL(cluster_border_kernel, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
  }
  MV_HIP(hipGetLastError());
  {
    ProfScope ps(c, "cluster_label", 21.0 * n);
    size_t tb = scan_bytes;
    MV_HIP(rocprim::exclusive_scan(S.tmp.p, tb, flag, pos, 0, NN, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(cluster_label_kernel, dim3(grid_of(n, VT)), dim3(VT), 0, st, S.core, root, flag, pos, n, S.label, S.size, d_ctl);
  }
  MV_HIP(hipGetLastError());
  // the sizes come back whole (C <= n is not known yet): the select rule and the largest cluster are the host's
  MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(ClCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipMemcpyAsync(S.pin.p + 256, S.size, 4 * NN, hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  const int C = h_ctl->clusters;
  if (C < 0 || C > n || h_ctl->core + h_ctl->border + h_ctl->noise != n) {
    set_error("cluster: %d clusters, %d + %d + %d of %d points", C, h_ctl->core, h_ctl->border, h_ctl->noise, n);
    return MVICP_ERR_INTERNAL;
  }
  const int* hs = reinterpret_cast<const int*>(S.pin.p + 256);
  S.h_size.assign(hs, hs + C);
  R.clusters = C; R.core = h_ctl->core; R.border = h_ctl->border; R.noise = h_ctl->noise;
  for (int k = 0; k < C; ++k)
    if (hs[k] > R.largest) { R.largest = hs[k]; R.largest_label = k; }   // (strictly larger: the lowest label among equals)
  if (stats) *stats = R;
  S.n = n; S.clusters = C; S.frame = frame;
  return C;
}

long long cluster_select(mvicp_ctx* c, const FrameDev& f, long long min_size, long long max_clusters) {
  ClusterStage& S = c->clu;
  S.sel.drop();   // (the last selection ends here, also when the keep rule fails)
  const int n = (int)S.n, C = (int)S.clusters;
  const unsigned char* d_keep = S.keep;
  const int* label = S.label;
  if (C > 0) {
    unsigned char* h_keep = reinterpret_cast<unsigned char*>(S.pin.p + 256);
    MV_CHECK(mvicp_cluster_keep_rule(C, S.h_size.data(), min_size, max_clusters, h_keep));
    MV_HIP(hipMemcpyAsync(S.keep, h_keep, (size_t)C, hipMemcpyHostToDevice, c->stream));
  }
  // (the flags are this stage's to write, and the cluster_compact scope has always covered the kernel that writes them: so it is launched
  // from inside select_rows, under the scope, and not before the call)
  return select_rows(c, S.sel, f, "cluster select", "cluster_compact", f.nor ? 112.0 : 64.0, nullptr, 0, label, [=](hipStream_t st, int* flag) {
    hipLaunchKernelGGL(cluster_keep_kernel, dim3(grid_of(n, VT)), dim3(VT), 0, st, label, d_keep, n, flag);
  });
}

}  // namespace mvicp
