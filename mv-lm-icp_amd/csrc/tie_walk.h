// nanoflann's exact 1-NN search, restated over kdvisit.h's tree — the walk of the tie fix-up (nn_tie.hip), as a header so that the host can
// compile the very function the kernel runs (tests/kdvisit_harness.cpp, tests/sanitize_harness.cpp).
//
// tie_walk restates findNeighbors / searchLevel for a result set of capacity 1 (include/nanoflann.hpp:900-911, 1199-1247, 75-134 without
// NANOFLANN_FIRST_MATCH): initial per-axis distances to the root box (computeInitialDistances, :1177-1193), leaf points replace the best
// only when strictly nearer (:1209), the near child is the low one iff (val - divlow) + (val - divhigh) < 0 (:1222-1233), the far child
// is entered iff mindistsq * epsError <= worstDist with epsError = 1 (:1240), with the reference's expressions in the reference's order.
// Every including TU must be built with -ffp-contract=off: the sums below are the reference's plain-SSE2 ones only without contraction.
//
// The recursion is an explicit stack of pending subtrees, supplied by the caller.  A descent pops one entry and pushes two per inner node,
// so the walk never holds more entries than the tree has levels (build_visit_tree's return value): a caller that passes cap >= levels
// cannot be truncated.  A stack that is too small all the same is reported (TIE_WALK_TRUNCATED), never answered from.
#pragma once
#include <cstddef>

#include "kdvisit.h"

namespace mvicp {

struct TiePending { int node, first; double mind, d0, d1, d2; };   // a subtree still to enter, with the state searchLevel would enter it in

struct TieTree {
  const VisitNode* nodes; const int* ord;   // kdvisit.h's tree; slot -> original index
  const double* pts;                        // the points, ORIGINAL order
  const double* box;                        // root bounding box: lo[3] | hi[3]
};

constexpr int TIE_WALK_TRUNCATED = -2;

// nanoflann's answer for one query: original index of the neighbour (-1: empty tree) and its squared distance.  `st`: room for `cap`
// pending entries.  TIE_WALK_TRUNCATED: the tree has more levels than cap — *d2_out is not an answer then.
MV_HD inline int tie_walk(const TieTree& T, double qx, double qy, double qz, TiePending* st, int cap, double* d2_out) {
  int sp = 0;
  double worst = 1.7976931348623157e308;   // KNNResultSet::init: dists[capacity - 1] = max
  int bi = -1;
  if (cap < 1) return TIE_WALK_TRUNCATED;
  {
    // computeInitialDistances: per axis the squared distance to the root box, summed in axis order
    const double q[3] = {qx, qy, qz};
    double d[3], s = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      d[a] = 0.0;
      if (q[a] < T.box[a]) d[a] = (q[a] - T.box[a]) * (q[a] - T.box[a]);
      if (q[a] > T.box[3 + a]) d[a] = (q[a] - T.box[3 + a]) * (q[a] - T.box[3 + a]);
      s = s + d[a];
    }
    st[sp++] = TiePending{0, 0, s, d[0], d[1], d[2]};
  }
  while (sp > 0) {
    TiePending f = st[--sp];
    if (f.node < 0) {
      // a far child: entered iff mindistsq * epsError <= worstDist NOW — i.e. after the near subtree (everything that was above this entry
      // on the stack) has been searched, exactly where the recursive form evaluates the test
      if (!(f.mind <= worst)) continue;
      f.node = -f.node - 1;
    }
    const VisitNode nd = T.nodes[f.node];
    if (nd.axis < 0) {                       // leaf: slots [first, split)
      for (int s = f.first; s < nd.split; ++s) {
        const int idx = T.ord[s];
        const double* p = T.pts + 3 * (size_t)idx;
        const double e0 = qx - p[0], e1 = qy - p[1], e2 = qz - p[2];
        const double dist = (e0 * e0 + e1 * e1) + e2 * e2;
        if (dist < worst) { worst = dist; bi = idx; }
      }
      continue;
    }
    const double val = nd.axis == 0 ? qx : nd.axis == 1 ? qy : qz;
    const double diff1 = val - nd.lo_cut, diff2 = val - nd.hi_cut;
    const bool low_first = diff1 + diff2 < 0.0;
    const double cut = low_first ? diff2 * diff2 : diff1 * diff1;   // accum_dist(val, divhigh | divlow)
    const double dst = nd.axis == 0 ? f.d0 : nd.axis == 1 ? f.d1 : f.d2;
    TiePending far = f;
    far.node = -(low_first ? nd.right : f.node + 1) - 1;   // (negative: "test mindistsq when popped"; child ids are >= 1)
    far.first = low_first ? nd.split : f.first;
    far.mind = (f.mind + cut) - dst;
    if (nd.axis == 0) far.d0 = cut; else if (nd.axis == 1) far.d1 = cut; else far.d2 = cut;
    TiePending near = f;
    near.node = low_first ? f.node + 1 : nd.right;
    near.first = low_first ? f.first : nd.split;
    if (sp + 2 > cap) return TIE_WALK_TRUNCATED;   // (more levels than the caller said: no answer)
    st[sp++] = far;
    st[sp++] = near;
  }
  *d2_out = worst;
  return bi;
}

}  // namespace mvicp
