// Thin extern "C" layer over mv-lm-icp_amd/csrc/lin_table.h for tests/test_lin_launch_table.py (TEST INFRASTRUCTURE, host only: no HIP, no GPU).
#include "../mv-lm-icp_amd/csrc/lin_table.h"

extern "C" {

// the launch table for edges with n_src[e] source points each in chunks of `chunk`.  -> the number of entries; at most cap of them are written
int lin_table(int n_edges, const int* src, const int* n_src, int chunk, int interleave, int tail_last, int cap, int* chunk_edge, int* chunk_start) {
  std::vector<long long> n(n_src, n_src + n_edges);
  std::vector<int> ce, cs;
  mvicp::lin_launch_table(n_edges, src, n.data(), chunk, interleave != 0, tail_last != 0, ce, cs);
  for (int i = 0; i < (int)ce.size() && i < cap; ++i) { chunk_edge[i] = ce[i]; chunk_start[i] = cs[i]; }
  return (int)ce.size();
}

}  // extern "C"
