// The order-preserving compaction of the stages that select rows of a stored cloud (outlier.hip, cluster.hip, plane.hip, boundary.hip): after an
// exclusive scan of the 0 / 1 flags over the original index, one lane per point stores its row at its rank, so the kept rows come out
// in ascending original index.  Plain vector stores only; the last lane leaves the number kept.
#pragma once
#include <hip/hip_runtime.h>

namespace mvicp {

constexpr int kCompactRowsThreads = 256;

// NRM: the cloud has normals (nor / nrm are read / written); LAB: a per-point label travels with the row (label / klabel)
template <bool NRM, bool LAB>
__global__ __launch_bounds__(kCompactRowsThreads) void compact_rows_kernel(const double* __restrict__ pts, const double* __restrict__ nor, const int* __restrict__ label,
                                                                           const int* __restrict__ flag, const int* __restrict__ pos, int n, double* __restrict__ xyz,
                                                                           double* __restrict__ nrm, int* __restrict__ idx, int* __restrict__ klabel, int* __restrict__ kept) {
  const int i = blockIdx.x * kCompactRowsThreads + threadIdx.x;
  if (i >= n) return;
  const int f = flag[i], o = pos[i];   // o <= i < n: inside the n-row destinations
  if (f) {
#pragma unroll
    for (int a = 0; a < 3; ++a) xyz[3 * (size_t)o + a] = pts[3 * (size_t)i + a];
    if (NRM) {
#pragma unroll
      for (int a = 0; a < 3; ++a) nrm[3 * (size_t)o + a] = nor[3 * (size_t)i + a];
    }
    idx[o] = i;
    if (LAB) klabel[o] = label[i];
  }
  if (i == n - 1) *kept = o + f;
}

// flag[i] = (flags[i] == want) as an int: what the scan and the compaction read, from a stage's flag bytes (plane.hip, boundary.hip).  A
// template only so that the header may define it
template <int THREADS = kCompactRowsThreads>
__global__ __launch_bounds__(THREADS) void rows_wanted_kernel(const unsigned char* __restrict__ flags, int n, int want, int* __restrict__ flag) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i < n) flag[i] = flags[i] == want ? 1 : 0;
}

// the launch: flag and pos are n ints each, pos = the exclusive scan of flag
template <bool LAB>
inline void compact_rows(hipStream_t st, const double* pts, const double* nor, const int* label, const int* flag, const int* pos, int n, double* xyz, double* nrm, int* idx,
                         int* klabel, int* kept) {
  const dim3 grid((unsigned int)((n + kCompactRowsThreads - 1) / kCompactRowsThreads)), block(kCompactRowsThreads);
  if (nor) hipLaunchKernelGGL((compact_rows_kernel<true, LAB>), grid, block, 0, st, pts, nor, label, flag, pos, n, xyz, nrm, idx, klabel, kept);
  else hipLaunchKernelGGL((compact_rows_kernel<false, LAB>), grid, block, 0, st, pts, nor, label, flag, pos, n, xyz, nrm, idx, klabel, kept);
}

}  // namespace mvicp
