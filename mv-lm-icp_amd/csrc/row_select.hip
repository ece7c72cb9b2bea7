// The order-preserving compaction of the stages that select rows of a stored cloud (row_select.h): after an exclusive scan of the 0 / 1
// flags over the original index, one lane per point stores its row at its rank, so the kept rows come out in ascending original index.
// Plain vector stores only; the last lane leaves the number kept.  No floating-point arithmetic: rows are copied.  DESIGN.md §3.8.
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "row_select.h"

namespace mvicp {

namespace {

constexpr int kThreads = 256;

// NRM: the cloud has normals (nor / nrm are read / written); LAB: a per-point label travels with the row (label / klabel)
template <bool NRM, bool LAB>
__global__ __launch_bounds__(kThreads) void compact_rows_kernel(const double* __restrict__ pts, const double* __restrict__ nor, const int* __restrict__ label,
                                                                const int* __restrict__ flag, const int* __restrict__ pos, int n, double* __restrict__ xyz,
                                                                double* __restrict__ nrm, int* __restrict__ idx, int* __restrict__ klabel, int* __restrict__ kept) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
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

// flag[i] = (flags[i] == want) as an int: what the scan and the compaction read, from a stage's flag bytes
__global__ __launch_bounds__(kThreads) void rows_wanted_kernel(const unsigned char* __restrict__ flags, int n, int want, int* __restrict__ flag) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) flag[i] = flags[i] == want ? 1 : 0;
}

template <bool LAB>
void compact_rows(hipStream_t st, const FrameDev& f, const int* label, const RowSelection& s, int* kept) {
  const dim3 grid(grid_of(f.n, kThreads)), block(kThreads);
  if (f.nor) hipLaunchKernelGGL((compact_rows_kernel<true, LAB>), grid, block, 0, st, f.pts, f.nor, label, s.flag, s.rank, f.n, s.xyz, s.nrm, s.idx, s.klabel, kept);
  else hipLaunchKernelGGL((compact_rows_kernel<false, LAB>), grid, block, 0, st, f.pts, f.nor, label, s.flag, s.rank, f.n, s.xyz, s.nrm, s.idx, s.klabel, kept);
}

}  // namespace

// one buffer [kept word | flag | rank | xyz | nrm | idx | klabel], the scan's storage and the pinned word, for selections among n rows
int RowSelection::reserve(long long n, bool labels, hipStream_t st) {
  drop();
  rows = -1;
  const size_t N = (size_t)n;
  size_t o = 256;
  auto take = [&](size_t b) { const size_t at = o; o += align256(std::max<size_t>(b, 1)); return at; };
  const size_t o_flag = take(4 * N), o_rank = take(4 * N), o_xyz = take(24 * N), o_nrm = take(24 * N), o_idx = take(4 * N), o_lab = labels ? take(4 * N) : 0;
  MV_CHECK(dev.reserve(o));
  MV_CHECK(pin.reserve(256));
  char* D = dev.p;
  flag = reinterpret_cast<int*>(D + o_flag); rank = reinterpret_cast<int*>(D + o_rank);
  xyz = reinterpret_cast<double*>(D + o_xyz); nrm = reinterpret_cast<double*>(D + o_nrm);
  idx = reinterpret_cast<int*>(D + o_idx); klabel = labels ? reinterpret_cast<int*>(D + o_lab) : nullptr;
  size_t scan_bytes = 0;
  MV_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag, rank, 0, N, rocprim::plus<int>(), st));
  MV_CHECK(tmp.reserve(std::max<size_t>(scan_bytes, 256)));
  rows = n;
  return MVICP_OK;
}

long long select_rows(mvicp_ctx* c, RowSelection& sel, const FrameDev& f, const char* stage, const char* scope, double bytes_per_row, const unsigned char* flags,
                      int want, const int* label, const std::function<void(hipStream_t, int*)>& write_flags) {
  sel.drop();   // (the last selection ends here; a failed call leaves none behind)
  const int n = f.n;
  if (n == 0) { sel.kept = 0; sel.has_normals = f.nor ? 1 : 0; return 0; }
  if (sel.rows != n) { set_error("%s: the selection is reserved for %lld rows, the frame has %d", stage, sel.rows, n); return MVICP_ERR_INTERNAL; }
  if (label && !sel.klabel) { set_error("%s: the selection is reserved without labels", stage); return MVICP_ERR_INTERNAL; }
  hipStream_t st = c->stream;
  int* d_kept = reinterpret_cast<int*>(sel.dev.p);
  int* h_kept = reinterpret_cast<int*>(sel.pin.p);
  {
    ProfScope ps(c, scope, bytes_per_row * n);
    if (flags) hipLaunchKernelGGL(rows_wanted_kernel, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, st, flags, n, want, sel.flag);
    else if (write_flags) write_flags(st, sel.flag);
    size_t tb = sel.tmp.cap;
    MV_HIP(rocprim::exclusive_scan(sel.tmp.p, tb, sel.flag, sel.rank, 0, (size_t)n, rocprim::plus<int>(), st));
    if (label) compact_rows<true>(st, f, label, sel, d_kept);
    else compact_rows<false>(st, f, label, sel, d_kept);
  }
  MV_HIP(hipGetLastError());
  MV_HIP(hipMemcpyAsync(h_kept, d_kept, sizeof(int), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  const int kept = *h_kept;
  if (kept < 0 || kept > n) { set_error("%s: %d kept of %d", stage, kept, n); return MVICP_ERR_INTERNAL; }
  sel.kept = kept; sel.has_normals = f.nor ? 1 : 0;
  return kept;
}

}  // namespace mvicp
