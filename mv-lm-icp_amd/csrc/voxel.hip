// Voxel-grid reduction (mvicp_voxel_grid): the points of one or several frames, at given poses, reduced to one point per occupied
// voxel.  The result is a pure function of the inputs, bit for bit (the contract is stated in include/mvicp.h; tests/voxelref.py is
// its numpy form).  DESIGN.md §3.7.
//
// Passes, all on the context's stream:
//   1  cells   one lane per input point (position `seq` in the input sequence): gather p, w = R p + t in the rounded operations of the
//              contract, q = w / voxel (IEEE division), cell = floor(q) as int32; a quotient that is non-finite or >= 2^31 in magnitude
//              raises one flag.  Per-workgroup min / max of the cells, six integer atomics per workgroup.
//      -- host wait: 6 ints + flag; the host checks the key range and chooses the number of key bits --
//   2  keys    64-bit key ((cz - cmin_z) d_y + (cy - cmin_y)) d_x + (cx - cmin_x), value = seq
//   3  sort    rocprim::radix_sort_pairs over the bits the key range needs.  It is stable, so inside a voxel seq stays ascending.
//   4  runs    head flags, exclusive scan, run starts; m = number of runs
//      -- host wait: m; the result arrays are allocated --
//   5  permute (option "voxel_permute", default 1) one lane per SORTED position: gather p (and n) through seq, transform, store w (and
//              R n) in sorted order, so that the random gather runs with one lane per point and the reduction reads rows next to each other
//   6  reduce  one lane per voxel walks its run in ascending seq: s = +0.0; s = s + w.  The order of summation is the contract, so this
//              is "store once, sum per destination in a fixed order", not atomics.  With voxel_permute = 0 the lane re-gathers p through
//              seq and recomputes w: the same expression, hence the same bits.
// A run of thousands of points (a voxel larger than the cloud) is summed by ONE lane, sequentially, by contract: correct, not fast.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"

namespace mvicp {

namespace {

constexpr int VT = 256;   // threads per workgroup

struct alignas(16) VoxSrc {   // one selected, non-empty frame
  const double* pts;          // n x 3, original order
  const double* nor;          // n x 3 or null
  double xf[12];              // R (9, column-major) t (3)
  int off, n;                 // first position in the input sequence, number of points
};
static_assert(sizeof(VoxSrc) == 128, "VoxSrc layout");

struct VoxCtl { int cmin[3], cmax[3], bad, m; };

// the source whose range holds `seq`: the last one with off <= seq (off[0] = 0, strictly increasing: empty frames are not listed)
__device__ __forceinline__ int find_src(const VoxSrc* __restrict__ S, int n_src, int seq) {
  int lo = 0, hi = n_src - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (S[mid].off <= seq) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// w_c = ((R[c,0] p0 + R[c,1] p1) + R[c,2] p2) + t_c, every operation rounded on its own (the first line of xf_point, nn_metric.h)
__device__ __forceinline__ void world_point(const double* __restrict__ x, double p0, double p1, double p2, double* w) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    w[i] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x[i], p0), __dmul_rn(x[i + 3], p1)), __dmul_rn(x[i + 6], p2)), x[9 + i]);
}
__device__ __forceinline__ void world_normal(const double* __restrict__ x, double n0, double n1, double n2, double* m) {
#pragma unroll
  for (int i = 0; i < 3; ++i) m[i] = __dadd_rn(__dadd_rn(__dmul_rn(x[i], n0), __dmul_rn(x[i + 3], n1)), __dmul_rn(x[i + 6], n2));
}

// point `seq` of the input sequence in world coordinates (and its normal when NRM)
template <bool NRM>
__device__ __forceinline__ void load_world(const VoxSrc* __restrict__ S, int n_src, int seq, int with_pose, double* w, double* m) {
  const VoxSrc& s = S[find_src(S, n_src, seq)];
  const size_t k = 3 * (size_t)(seq - s.off);
  const double p0 = s.pts[k], p1 = s.pts[k + 1], p2 = s.pts[k + 2];
  if (with_pose) world_point(s.xf, p0, p1, p2, w);
  else { w[0] = p0; w[1] = p1; w[2] = p2; }
  if (NRM) {
    const double n0 = s.nor[k], n1 = s.nor[k + 1], n2 = s.nor[k + 2];
    if (with_pose) world_normal(s.xf, n0, n1, n2, m);
    else { m[0] = n0; m[1] = n1; m[2] = n2; }
  }
}

__global__ __launch_bounds__(VT) void vox_cell_kernel(const VoxSrc* __restrict__ S, int n_src, int N, int with_pose, double h, int* __restrict__ cells,
                                                      VoxCtl* __restrict__ ctl) {
  __shared__ int s_lo[VT / 64][3], s_hi[VT / 64][3];
  const int i = blockIdx.x * VT + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  bool bad = false;
  if (i < N) {
    double w[3];
    load_world<false>(S, n_src, i, with_pose, w, nullptr);
    int c[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double q = __ddiv_rn(w[a], h);
      if (!(fabs(q) < 2147483648.0)) bad = true;   // (a NaN fails the comparison too)
      else c[a] = (int)floor(q);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) cells[3 * (size_t)i + a] = c[a];
    if (!bad) {
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = hi[a] = c[a];
    }
  }
  if (__ballot(bad) != 0ull && lane == 0) atomicOr(&ctl->bad, 1);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], x, 64)); hi[a] = max(hi[a], __shfl_xor(hi[a], x, 64)); }
  if (lane == 0)
    for (int a = 0; a < 3; ++a) { s_lo[wave][a] = lo[a]; s_hi[wave][a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    int l = s_lo[0][a], u = s_hi[0][a];
    for (int k = 1; k < VT / 64; ++k) { l = min(l, s_lo[k][a]); u = max(u, s_hi[k][a]); }
    if (l <= u) { atomicMin(&ctl->cmin[a], l); atomicMax(&ctl->cmax[a], u); }
  }
}

__global__ __launch_bounds__(VT) void vox_key_kernel(const int* __restrict__ cells, int N, int cx0, int cy0, int cz0, unsigned long long dx, unsigned long long dy,
                                                     unsigned long long* __restrict__ key, int* __restrict__ seq) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= N) return;
  const unsigned long long x = (unsigned long long)((long long)cells[3 * (size_t)i] - cx0), y = (unsigned long long)((long long)cells[3 * (size_t)i + 1] - cy0),
                           z = (unsigned long long)((long long)cells[3 * (size_t)i + 2] - cz0);
  key[i] = (z * dy + y) * dx + x;
  seq[i] = i;
}

__global__ __launch_bounds__(VT) void vox_head_kernel(const unsigned long long* __restrict__ key, int N, int* __restrict__ head) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i < N) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// rstart[v] = first sorted position of run v, rstart[m] = N; m itself to the control block
__global__ __launch_bounds__(VT) void vox_start_kernel(const int* __restrict__ head, const int* __restrict__ rid, int N, int* __restrict__ rstart, VoxCtl* __restrict__ ctl) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= N) return;
  if (head[i]) rstart[rid[i]] = i;
  if (i == N - 1) { const int m = rid[i] + head[i]; rstart[m] = N; ctl->m = m; }
}

template <bool NRM>
__global__ __launch_bounds__(VT) void vox_permute_kernel(const VoxSrc* __restrict__ S, int n_src, int N, int with_pose, const int* __restrict__ seq, double* __restrict__ W,
                                                         double* __restrict__ M) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= N) return;
  double w[3], m[3];
  load_world<NRM>(S, n_src, seq[i], with_pose, w, m);
#pragma unroll
  for (int a = 0; a < 3; ++a) W[3 * (size_t)i + a] = w[a];
  if (NRM) {
#pragma unroll
    for (int a = 0; a < 3; ++a) M[3 * (size_t)i + a] = m[a];
  }
}

// one lane per voxel: the sequential sums of its run, in ascending seq
template <bool NRM, bool PERM>
__global__ __launch_bounds__(VT) void vox_reduce_kernel(const VoxSrc* __restrict__ S, int n_src, int with_pose, const int* __restrict__ seq, const double* __restrict__ W,
                                                        const double* __restrict__ M, const int* __restrict__ rstart, int m_runs, double* __restrict__ xyz,
                                                        double* __restrict__ nrm, int* __restrict__ cnt) {
  const int v = blockIdx.x * VT + threadIdx.x;
  if (v >= m_runs) return;
  const int lo = rstart[v], hi = rstart[v + 1];
  double s[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
  for (int i = lo; i < hi; ++i) {
    double w[3], m[3];
    if (PERM) {
#pragma unroll
      for (int a = 0; a < 3; ++a) w[a] = W[3 * (size_t)i + a];
      if (NRM) {
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = M[3 * (size_t)i + a];
      }
    } else {
      load_world<NRM>(S, n_src, seq[i], with_pose, w, m);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = __dadd_rn(s[a], w[a]);
    if (NRM) {
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] = __dadd_rn(t[a], m[a]);
    }
  }
  const int n = hi - lo;
  const double dn = (double)n;
#pragma unroll
  for (int a = 0; a < 3; ++a) xyz[3 * (size_t)v + a] = __ddiv_rn(s[a], dn);
  cnt[v] = n;
  if (NRM) {
    const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(t[0], t[0]), __dmul_rn(t[1], t[1])), __dmul_rn(t[2], t[2])));
    const bool ok = len > 0.0 && len < INFINITY;   // (false for NaN)
#pragma unroll
    for (int a = 0; a < 3; ++a) nrm[3 * (size_t)v + a] = ok ? __ddiv_rn(t[a], len) : 0.0;
  }
}

}  // namespace

long long voxel_reduce(mvicp_ctx* c, int n_sel, const int* sel, const double* poses, double voxel, int* has_normals) {
  c->vox.drop_result();   // (the last result lives until the next grid call)
  // the input sequence: the selected frames in order, empty ones left out
  std::vector<VoxSrc> srcs;
  long long total = 0;
  bool normals = true;
  for (int k = 0; k < n_sel; ++k) {
    const FrameDev& f = c->frames[sel[k]];
    if (f.n == 0) continue;
    VoxSrc s;
    std::memset(&s, 0, sizeof(s));
    s.pts = f.pts; s.nor = f.nor; s.off = (int)total; s.n = f.n;
    if (poses) {
      const double* P = poses + 16 * (size_t)sel[k];
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) s.xf[i + 3 * j] = P[i + 4 * j];
      for (int i = 0; i < 3; ++i) s.xf[9 + i] = P[12 + i];
    }
    if (!f.nor) normals = false;
    total += f.n;
    srcs.push_back(s);
  }
  if (has_normals) *has_normals = normals ? 1 : 0;
  c->vox.has_normals = normals ? 1 : 0;
  if (total == 0) { c->vox.m = 0; return 0; }
  const int N = (int)total, n_src = (int)srcs.size(), with_pose = poses ? 1 : 0;
  const bool permute = c->voxel_permute != 0;
  hipStream_t st = c->stream;

  // scratch: [sources | control | cells 3N int (later: head N, run id N) | key a, b | seq a, b | run starts N + 1 | w, m in sorted order]
  const size_t NN = (size_t)N;
  const size_t off_ctl = align256(sizeof(VoxSrc) * n_src), off_cells = off_ctl + 256, off_ka = off_cells + align256(12 * NN), off_kb = off_ka + align256(8 * NN);
  const size_t off_sa = off_kb + align256(8 * NN), off_sb = off_sa + align256(4 * NN), off_rs = off_sb + align256(4 * NN), off_w = off_rs + align256(4 * (NN + 1));
  const size_t off_m = off_w + (permute ? align256(24 * NN) : 0), bytes = off_m + (permute && normals ? align256(24 * NN) : 0);
  MV_CHECK(c->vox.scratch.reserve(bytes));
  MV_CHECK(c->vox.pin.reserve(off_cells));
  char* D = c->vox.scratch.p;
  const VoxSrc* d_src = reinterpret_cast<const VoxSrc*>(D);
  VoxCtl* d_ctl = reinterpret_cast<VoxCtl*>(D + off_ctl);
  int* cells = reinterpret_cast<int*>(D + off_cells);
  int* head = cells; int* rid = cells + NN;   // (the cells are dead once the keys exist)
  unsigned long long* key_a = reinterpret_cast<unsigned long long*>(D + off_ka);
  unsigned long long* key_b = reinterpret_cast<unsigned long long*>(D + off_kb);
  int* seq_a = reinterpret_cast<int*>(D + off_sa); int* seq_b = reinterpret_cast<int*>(D + off_sb);
  int* rstart = reinterpret_cast<int*>(D + off_rs);
  double* W = permute ? reinterpret_cast<double*>(D + off_w) : nullptr;
  double* M = permute && normals ? reinterpret_cast<double*>(D + off_m) : nullptr;

  std::memcpy(c->vox.pin.p, srcs.data(), sizeof(VoxSrc) * n_src);
  VoxCtl* h_ctl = reinterpret_cast<VoxCtl*>(c->vox.pin.p + off_ctl);
  for (int a = 0; a < 3; ++a) { h_ctl->cmin[a] = INT_MAX; h_ctl->cmax[a] = INT_MIN; }
  h_ctl->bad = 0; h_ctl->m = 0;
  MV_HIP(hipMemcpyAsync(D, c->vox.pin.p, off_ctl + sizeof(VoxCtl), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(vox_cell_kernel, dim3(grid_of(N, VT)), dim3(VT), 0, st, d_src, n_src, N, with_pose, voxel, cells, d_ctl);
  MV_HIP(hipGetLastError());
  MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(VoxCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (h_ctl->bad) { set_error("a coordinate / voxel is not finite or >= 2^31 in magnitude (voxel %g too small for the coordinates?)", voxel); return MVICP_ERR_ARG; }
  unsigned long long d[3];
  for (int a = 0; a < 3; ++a) d[a] = (unsigned long long)((long long)h_ctl->cmax[a] - (long long)h_ctl->cmin[a] + 1);   // 1 .. 2^32
  const unsigned __int128 cells_total = (unsigned __int128)d[0] * d[1] * d[2];   // < 2^96
  if (cells_total >= ((unsigned __int128)1 << 62)) {
    set_error("voxel too small for the extent (%llu x %llu x %llu cells)", d[0], d[1], d[2]);
    return MVICP_ERR_ARG;
  }
  int bits = 1;
  while (bits < 62 && ((unsigned long long)1 << bits) < (unsigned long long)cells_total) ++bits;   // keys are < cells_total <= 2^bits

  size_t sort_bytes = 0, scan_bytes = 0;
  MV_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, key_a, key_b, seq_a, seq_b, NN, 0, bits, st));
  MV_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, head, rid, 0, NN, rocprim::plus<int>(), st));
  size_t tmp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 256);
  MV_CHECK(c->vox.tmp.reserve(tmp_bytes));

  hipLaunchKernelGGL(vox_key_kernel, dim3(grid_of(N, VT)), dim3(VT), 0, st, cells, N, h_ctl->cmin[0], h_ctl->cmin[1], h_ctl->cmin[2], d[0], d[1], key_a, seq_a);
  MV_HIP(hipGetLastError());
  size_t tb = sort_bytes;
  MV_HIP(rocprim::radix_sort_pairs(c->vox.tmp.p, tb, key_a, key_b, seq_a, seq_b, NN, 0, bits, st));
  hipLaunchKernelGGL(vox_head_kernel, dim3(grid_of(N, VT)), dim3(VT), 0, st, key_b, N, head);
  MV_HIP(hipGetLastError());
  tb = scan_bytes;
  MV_HIP(rocprim::exclusive_scan(c->vox.tmp.p, tb, head, rid, 0, NN, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(vox_start_kernel, dim3(grid_of(N, VT)), dim3(VT), 0, st, head, rid, N, rstart, d_ctl);
  MV_HIP(hipGetLastError());
  MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(VoxCtl), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  const int m = h_ctl->m;
  if (m < 1 || m > N) { set_error("voxel grid: run count %d out of range [1, %d]", m, N); return MVICP_ERR_INTERNAL; }

  MV_HIP(hipMalloc((void**)&c->vox.xyz, sizeof(double) * 3 * (size_t)m));
  if (normals) MV_HIP(hipMalloc((void**)&c->vox.nrm, sizeof(double) * 3 * (size_t)m));
  MV_HIP(hipMalloc((void**)&c->vox.cnt, sizeof(int) * (size_t)m));
  if (permute) {
    if (normals) hipLaunchKernelGGL(vox_permute_kernel<true>, dim3(grid_of(N, VT)), dim3(VT), 0, st, d_src, n_src, N, with_pose, seq_b, W, M);
    else hipLaunchKernelGGL(vox_permute_kernel<false>, dim3(grid_of(N, VT)), dim3(VT), 0, st, d_src, n_src, N, with_pose, seq_b, W, M);
    MV_HIP(hipGetLastError());
  }
#define MV_VOX_REDUCE(NRM, PERM) \
  hipLaunchKernelGGL((vox_reduce_kernel<NRM, PERM>), dim3(grid_of(m, VT)), dim3(VT), 0, st, d_src, n_src, with_pose, seq_b, W, M, rstart, m, c->vox.xyz, c->vox.nrm, c->vox.cnt)
  if (normals) { if (permute) MV_VOX_REDUCE(true, true); else MV_VOX_REDUCE(true, false); }
  else { if (permute) MV_VOX_REDUCE(false, true); else MV_VOX_REDUCE(false, false); }
#undef MV_VOX_REDUCE
  MV_HIP(hipGetLastError());
  MV_HIP(hipStreamSynchronize(st));
  c->vox.m = m;
  return m;
}

}  // namespace mvicp
