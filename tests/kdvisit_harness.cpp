// Host-only harness around mv-lm-icp_amd/csrc/kdvisit.h (the tie order of Frame::recomputeNormals' k-NN): brute-force k-NN of every point
// of a cloud with the metric of include/frame.h:70-76 and equal distances ordered by visited_before().  Compiled by
// tests/test_knn_tie_order.py with -I <repo>/mv-lm-icp_amd/csrc; no GPU involved.
// tie_walk_emul: the 1-NN tie fix-up's own walk (csrc/tie_walk.h, the function nn_tie.hip's kernels run) compiled for the host, over the same tree
// (tests/test_tie_walk_cpu.py).
#include "kdvisit.h"
#include "tie_walk.h"
#include <cstdio>
using namespace mvicp;
extern "C" int knn_emul(const double* xyz, int n, int K, int* out) {
  std::vector<VisitNode> nodes; std::vector<int> slot;
  build_visit_tree(xyz, n, nodes, slot);
  VisitTree T{nodes.data(), slot.data()};
  #pragma omp parallel for schedule(dynamic,64)
  for (int i = 0; i < n; ++i) {
    const double qx = xyz[3*i], qy = xyz[3*i+1], qz = xyz[3*i+2];
    std::vector<double> bd(K, 1e300); std::vector<long long> bo(K, -1);
    for (int j = 0; j < n; ++j) {
      const double d0 = qx - xyz[3*j], d1 = qy - xyz[3*j+1], d2 = qz - xyz[3*j+2];
      const double d = d0*d0 + d1*d1 + d2*d2;
      double cd = d; long long co = j;
      if (!(cd < bd[K-1] || (cd == bd[K-1] && (bo[K-1] < 0 || visited_before(T, qx,qy,qz, co, bo[K-1]))))) continue;
      for (int t = 0; t < K; ++t) {
        if (cd < bd[t] || (cd == bd[t] && (bo[t] < 0 || visited_before(T, qx,qy,qz, co, bo[t])))) { std::swap(cd, bd[t]); std::swap(co, bo[t]); }
      }
    }
    for (int t = 0; t < K; ++t) out[(size_t)i*K+t] = (int)bo[t];
  }
  return (int)nodes.size();
}

// 1-NN of m queries against the cloud through tie_walk on build_visit_tree's tree.  cap <= 0: a stack of the tree's levels (what the product
// allocates); cap > 0: that many entries — a query whose walk needs more gets idx = TIE_WALK_TRUNCATED (d2 untouched).  Returns the levels.
extern "C" int tie_walk_emul(const double* xyz, int n, const double* q, int m, int cap, int* idx, double* d2) {
  std::vector<VisitNode> nodes; std::vector<int> slot;
  const int levels = build_visit_tree(xyz, n, nodes, slot);
  std::vector<int> ord(n);
  for (int i = 0; i < n; ++i) ord[slot[i]] = i;
  double box[6];
  for (int a = 0; a < 3; ++a) box[a] = box[3 + a] = xyz[a];
  for (int i = 1; i < n; ++i)
    for (int a = 0; a < 3; ++a) { const double v = xyz[3 * (size_t)i + a]; if (v < box[a]) box[a] = v; if (v > box[3 + a]) box[3 + a] = v; }
  const TieTree T{nodes.data(), ord.data(), xyz, box};
  const int use = cap > 0 ? cap : levels;
  std::vector<TiePending> st(use);
  for (int i = 0; i < m; ++i) idx[i] = tie_walk(T, q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2], st.data(), use, &d2[i]);
  return levels;
}
