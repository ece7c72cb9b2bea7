// The launch table of the linearize workgroups: which (edge, first correspondence) pair workgroup b of a launch works on.  Host-only, no device
// call: mvicp_set_graph fills the device's copy from it, and tests/lin_table_harness.cpp hands it to tests.  The table decides only the ORDER in
// which the chunks of a launch start.  A chunk's partial goes to the slot chunk_first[e] + k of its edge, and an entry whose start is not below the
// edge's count returns at once, so every order, with or without pads, gives the same blocks bit for bit.
//
// interleave ("lin_interleave"): the edges of one source cloud (consecutive in the edge list) read the same p (identity lists, lin_share_p).  Their
//   chunks are interleaved in groups of 8 — A0..A7, B0..B7, A8..A15, ... — so that chunk k of the second edge runs on the XCD (workgroup b runs on
//   XCD b % 8) that chunk k of the first edge ran on a moment ago: its piece of p is still in that XCD's L2.
// tail_last ("lin_tail_last"): the workgroups that start last run almost alone with two steps of loads in flight per lane: a full chunk there is a
//   latency-bound tail of the whole launch, a short chunk is not.  So every edge's partial last chunk moves behind all full chunks.  Its place in the
//   order above is KEPT, by a pad: every full chunk sits at the entry, and so on the XCD, where it sits without the option (a source cloud's run keeps
//   its length, and with it the rotation of the XCDs from one source to the next that spreads the load when the lists are only partly filled and the
//   upper chunks of every edge return at once).  The tail section keeps the interleave's property row-wise: 8 source clouds per batch, the last chunks
//   of their first edges, then of their second edges, ...; a place without a chunk holds a pad, so that the last chunks of two edges of one source
//   cloud sit a multiple of 8 apart.  Pads at the very end of the table are dropped.
// A PAD is an entry (e, n_all(e) * chunk): its start is at or past the edge's end (start >= n >= count).  Its slot expression chunk_first[e] + start /
//   chunk names the NEXT edge's first slot; that is harmless only because every accumulation kernel returns before any store when start >= count
//   (linearize.hip linearize_kernel, lin_normal.h linearize_normal_body: `if (start >= cnt) return;` ahead of everything else).  A kernel that were to
//   write its slot for an empty chunk would have to test for a pad first.
#pragma once
#include <algorithm>
#include <vector>

namespace mvicp {

// n[e]: the source points of edge e that this rank holds (0 for an edge of another rank); chunk > 0
inline void lin_launch_table(int E, const int* src, const long long* n, int chunk, bool interleave, bool tail_last, std::vector<int>& chunk_edge,
                             std::vector<int>& chunk_start) {
  chunk_edge.clear(); chunk_start.clear();
  auto n_all = [&](int e) { return (int)((n[e] + chunk - 1) / chunk); };
  auto n_full = [&](int e) { return (int)(n[e] / chunk); };
  std::vector<int> g0, g1;   // [g0[i], g1[i]): the edges of one source cloud (without the interleave: one edge)
  for (int e0 = 0; e0 < E;) {
    int e1 = e0 + 1;
    while (interleave && e1 < E && src[e1] == src[e0]) ++e1;
    g0.push_back(e0); g1.push_back(e1);
    e0 = e1;
  }
  for (size_t i = 0; i < g0.size(); ++i) {
    int maxc = 0;
    for (int e = g0[i]; e < g1[i]; ++e) maxc = std::max(maxc, n_all(e));
    for (int g = 0; g < maxc; g += 8)
      for (int e = g0[i]; e < g1[i]; ++e)
        for (int k = g; k < std::min(g + 8, n_all(e)); ++k) {
          chunk_edge.push_back(e);
          chunk_start.push_back((tail_last && k >= n_full(e)) ? n_all(e) * chunk : k * chunk);   // the partial chunk's place: a pad
        }
  }
  if (!tail_last) return;
  for (size_t b = 0; b < g0.size(); b += 8) {
    const size_t b1 = std::min(b + 8, g0.size());
    int rows = 0;
    for (size_t i = b; i < b1; ++i) rows = std::max(rows, g1[i] - g0[i]);
    for (int j = 0; j < rows; ++j)
      for (size_t i = b; i < b + 8; ++i) {
        const int e = i < b1 && g0[i] + j < g1[i] ? g0[i] + j : -1;
        if (e >= 0 && n_full(e) < n_all(e)) { chunk_edge.push_back(e); chunk_start.push_back(n_full(e) * chunk); }
        else if (rows > 1) { chunk_edge.push_back(0); chunk_start.push_back(n_all(0) * chunk); }   // (one row: nobody to stay 8 apart from)
      }
  }
  while (!chunk_edge.empty() && chunk_start.back() >= n[chunk_edge.back()]) { chunk_edge.pop_back(); chunk_start.pop_back(); }
}

}  // namespace mvicp
