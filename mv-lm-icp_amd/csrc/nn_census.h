// The work census of the NN kernels (profiling with nn_census only): per-wave slots of 8 counters that the search kernels fill, their
// reduction and the asynchronous hand-over to the host.  Internal linkage: one copy per translation unit that launches a search.
#pragma once
#include "common.h"

namespace mvicp {

namespace {

// sums the per-wave census slots (8 counters each) into out8 (zeroed by the caller); 64 workgroups, 8 atomics each
__global__ __launch_bounds__(256) void census_sum_kernel(const unsigned long long* __restrict__ stats, size_t slots, unsigned long long* __restrict__ out8) {
  __shared__ unsigned long long sh[8][256];
  unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += (size_t)gridDim.x * 256)
    for (int k = 0; k < 8; ++k) v[k] += stats[8 * i + k];
  for (int k = 0; k < 8; ++k) sh[k][threadIdx.x] = v[k];
  __syncthreads();
  if (threadIdx.x < 8) {
    unsigned long long s = 0;
    for (int i = 0; i < 256; ++i) s += sh[threadIdx.x][i];
    atomicAdd(&out8[threadIdx.x], s);
  }
}

// scratch for the per-wave census slots; null when the census is off
inline int census_scratch(mvicp_ctx* c, size_t slots, unsigned long long** d_stats) {
  *d_stats = nullptr;
  if (c->profile && c->nn_census) {
    const size_t need = sizeof(unsigned long long) * 8 * (slots + 1);
    if (need > c->census_bytes) {
      if (c->d_census) MV_HIP(hipFree(c->d_census));
      MV_HIP(hipMalloc((void**)&c->d_census, need));
      c->census_bytes = need;
    }
    *d_stats = (unsigned long long*)c->d_census;
    MV_HIP(hipMemsetAsync(*d_stats, 0, need, c->stream));
  }
  return MVICP_OK;
}

// census counters -> pinned memory, asynchronously; census_resolve() (api.cpp) folds them in after the caller's own wait (no extra sync).
// kind: which kernel's counters these are (0 grid, 1 tree only, 2 tile / matrix pipe, 3 cell staging)
inline int census_collect(mvicp_ctx* c, unsigned long long* d_stats, size_t slots, double nq, int kind, const char* scope) {
  if (!c->h_census) MV_HIP(hipHostMalloc((void**)&c->h_census, 8 * sizeof(unsigned long long), hipHostMallocDefault));
  hipLaunchKernelGGL(census_sum_kernel, dim3(64), dim3(256), 0, c->stream, d_stats, slots, d_stats + 8 * slots);
  MV_HIP(hipMemcpyAsync(c->h_census, d_stats + 8 * slots, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  c->census_pending = true; c->census_nq = nq; c->census_kind = kind; c->census_scope = scope;
  return MVICP_OK;
}

}  // namespace

}  // namespace mvicp
