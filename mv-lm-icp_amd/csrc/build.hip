// Device build of the per-cloud NN structures (mvicp_set_frame_device): the same arrays as the host build (nn_grid.hip build_grid,
// nn_tile.hip build_wide, nn_mfma.hip build_mfma), byte for byte, made from a cloud that is already in device memory.
//
//   validate + bbox     one reduction: finiteness, lo / hi per axis, max |p| (mvicp_set_frame's max_norm), max |coordinate|   (in the call)
//   cell size           the host's heuristic (build_common.h choose_grid) with its occupancy counts taken on the device: distinct cell keys
//                       inserted into an open-addressing set (atomicCAS), at most 5 counts
//   cell order          curve key of every point's cell, stable LSD radix sort of (key, index) -> run heads -> run list, downloaded; the
//                       hash table and the brick map are then made on the host from that list exactly as the host build makes them
//   k-d order           (grid_curve 2, n > 64) presorted, level-synchronous: the segment tree of kd_split is data-independent, so every
//                       level is one pass over all segments.  Each axis list holds the segment's points sorted by (coordinate, index); the
//                       first and last entries give the bounding box, the axis is chosen as kd_split chooses it, the left set is the first
//                       mid - lo entries of that axis' list, and all three lists are partitioned stably (flag pass, one scan, scatter)
//   gathers             spts / sidx / srec / crec / inv / snor
//   boxes               8-ary tree (leaves, then bottom-up), 64-wide hierarchy (tiles, then levels): one thread per box, the host's loop
//   matrix-pipe         one workgroup per block of FAN x LEAF points: ordered lo / hi reduction, centre, exact scale exponent, the shared
//                       per-point operand code (build_common.h mf_point), block maxima
// The only host waits: the bbox (finiteness), the occupancy counts, the run list, and the final download of sidx / inv.
#include <chrono>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "build_common.h"
#include "common.h"
#include "nn_tile_common.h"

namespace mvicp {

namespace {

constexpr int BT = 256;
constexpr int kBoundsParts = 256;

__device__ __forceinline__ double dmin_first(double cur, double v) { return v < cur ? v : cur; }   // std::min(cur, v)
__device__ __forceinline__ double dmax_first(double cur, double v) { return cur < v ? v : cur; }   // std::max(cur, v)
__device__ __forceinline__ float fmin_first(float cur, float v) { return v < cur ? v : cur; }
__device__ __forceinline__ float fmax_first(float cur, float v) { return cur < v ? v : cur; }

// ---- validate + bbox ---------------------------------------------------------------------------------------------------------------------
// Order-free quantities only: min / max VALUES (a +-0 bound gives the same grid), max_norm and max |x| (non-negative).
__global__ __launch_bounds__(BT) void bounds_kernel(const double* __restrict__ xyz, int n, DevBounds* __restrict__ part) {
  __shared__ DevBounds sh[BT];
  DevBounds b;
  for (int a = 0; a < 3; ++a) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
  b.max_norm = 0.0; b.maxabs = 0.0; b.wall_ms = 0.0; b.nonfinite = 0; b.pad = 0;
  for (int i = blockIdx.x * BT + threadIdx.x; i < n; i += gridDim.x * BT) {
    const double p0 = xyz[3 * (size_t)i], p1 = xyz[3 * (size_t)i + 1], p2 = xyz[3 * (size_t)i + 2];
    if (!isfinite(p0) || !isfinite(p1) || !isfinite(p2)) { b.nonfinite = 1; continue; }
    const double p[3] = {p0, p1, p2};
    for (int a = 0; a < 3; ++a) { b.lo[a] = fmin(b.lo[a], p[a]); b.hi[a] = fmax(b.hi[a], p[a]); b.maxabs = fmax(b.maxabs, fabs(p[a])); }
    b.max_norm = fmax(b.max_norm, sqrt(b_add(b_add(b_mul(p0, p0), b_mul(p1, p1)), b_mul(p2, p2))));
  }
  sh[threadIdx.x] = b;
  __syncthreads();
  for (int s = BT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      DevBounds& l = sh[threadIdx.x];
      const DevBounds& r = sh[threadIdx.x + s];
      for (int a = 0; a < 3; ++a) { l.lo[a] = fmin(l.lo[a], r.lo[a]); l.hi[a] = fmax(l.hi[a], r.hi[a]); }
      l.max_norm = fmax(l.max_norm, r.max_norm); l.maxabs = fmax(l.maxabs, r.maxabs); l.nonfinite |= r.nonfinite;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// ---- occupancy count: distinct cell keys ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void occupancy_kernel(const double* __restrict__ xyz, int n, HostGrid g, unsigned long long* __restrict__ set,
                                                       unsigned int mask, int shift, unsigned int* __restrict__ count) {
  const int i = blockIdx.x * BT + threadIdx.x;
  unsigned int added = 0;
  if (i < n) {
    int cc[3];
    cell_of(g, xyz + 3 * (size_t)i, cc);
    const unsigned long long key = cell_key(cc[0], cc[1], cc[2]);
    unsigned int s = hash_slot(key, shift) & mask;
    for (unsigned int probe = 0; probe <= mask; ++probe) {   // (the set has room for twice n keys: a free slot is always found)
      const unsigned long long prev = atomicCAS(&set[s], kEmptyKey, key);
      if (prev == kEmptyKey) { added = 1; break; }
      if (prev == key) break;
      s = (s + 1) & mask;
    }
  }
  const unsigned long long ballot = __ballot(added);
  if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(count, (unsigned int)__popcll(ballot));
}

// ---- cell order ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void curve_keys_kernel(const double* __restrict__ xyz, int n, HostGrid g, int curve, int hbits,
                                                        unsigned long long* __restrict__ mkey, unsigned long long* __restrict__ ckey, int* __restrict__ idx) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  int cc[3];
  cell_of(g, xyz + 3 * (size_t)i, cc);
  mkey[i] = curve == 0 ? morton3((unsigned)cc[0], (unsigned)cc[1], (unsigned)cc[2]) : hilbert3((unsigned)cc[0], (unsigned)cc[1], (unsigned)cc[2], hbits);
  ckey[i] = cell_key(cc[0], cc[1], cc[2]);
  idx[i] = i;
}

__global__ __launch_bounds__(BT) void run_heads_kernel(const unsigned long long* __restrict__ ckey, const int* __restrict__ corder, int n, int* __restrict__ head) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  head[i] = i == 0 || ckey[corder[i]] != ckey[corder[i - 1]];
}

// rid: exclusive scan of head.  Run r = [start[r], start[r + 1]) of the cell order
__global__ __launch_bounds__(BT) void run_starts_kernel(const int* __restrict__ head, const int* __restrict__ rid, int n, int* __restrict__ start, int* __restrict__ n_runs) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  if (head[i]) start[rid[i]] = i;
  if (i == n - 1) *n_runs = rid[i] + head[i];
}

__global__ __launch_bounds__(BT) void run_list_kernel(const unsigned long long* __restrict__ ckey, const int* __restrict__ corder, const int* __restrict__ start,
                                                      const int* __restrict__ n_runs, int n, HashEntry* __restrict__ runs) {
  const int r = blockIdx.x * BT + threadIdx.x;
  const int R = *n_runs;
  if (r >= R) return;
  const int s = start[r], e = r + 1 < R ? start[r + 1] : n;
  runs[r] = HashEntry{ckey[corder[s]], (unsigned)s, (unsigned)(e - s)};
}

// ---- k-d order -----------------------------------------------------------------------------------------------------------------------------
// coordinate -> radix key whose unsigned order is the comparator's order of kd_split (-0.0 and +0.0 equal: ties go to the index)
__global__ __launch_bounds__(BT) void coord_keys_kernel(const double* __restrict__ xyz, int n, int axis, unsigned long long* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const double v = xyz[3 * (size_t)i + axis];
  unsigned long long u = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);
  key[i] = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  idx[i] = i;
}

// kd_split's split position of the segment [lo, hi)
__device__ __forceinline__ int kd_mid(int lo, int hi) {
  const int m = hi - lo;
  const int units = m > 32 ? (m + 31) / 32 : m, unit = m > 32 ? 32 : 1;
  int left = 1;
  while (left * 2 < units) left *= 2;
  return lo + left * unit;
}

struct Lists { const int* l[3]; };
struct OutLists { int* l[3]; };
struct Int3 { int v[3]; };
struct Int3Sum {
  __host__ __device__ Int3 operator()(const Int3& a, const Int3& b) const { return Int3{{a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2]}}; }
};

__global__ __launch_bounds__(BT) void kd_flag_kernel(Lists L, const double* __restrict__ xyz, const int* __restrict__ seg_lo, const int* __restrict__ seg_hi,
                                                     int n, int* __restrict__ is_left) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j >= n) return;
  const int lo = seg_lo[j], hi = seg_hi[j];
  if (hi - lo <= 1) return;
  // the segment's box: first and last entry of each axis list (the axis choice compares extents only, so the sign of a zero bound is immaterial)
  double ext[3];
  for (int a = 0; a < 3; ++a) ext[a] = b_sub(xyz[3 * (size_t)L.l[a][hi - 1] + a], xyz[3 * (size_t)L.l[a][lo] + a]);
  int ax = 0;
  if (ext[1] > ext[ax]) ax = 1;
  if (ext[2] > ext[ax]) ax = 2;
  is_left[L.l[ax][j]] = j < kd_mid(lo, hi);
}

__global__ __launch_bounds__(BT) void kd_count_kernel(Lists L, const int* __restrict__ seg_lo, const int* __restrict__ seg_hi, const int* __restrict__ is_left,
                                                      int n, Int3* __restrict__ flags) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j >= n) return;
  Int3 f{{0, 0, 0}};
  if (seg_hi[j] - seg_lo[j] > 1)
    for (int a = 0; a < 3; ++a) f.v[a] = is_left[L.l[a][j]];
  flags[j] = f;
}

// stable partition of every segment of the three lists; scan = exclusive scan of kd_count_kernel's flags.  Positions move to the children.
__global__ __launch_bounds__(BT) void kd_scatter_kernel(Lists L, OutLists O, int* __restrict__ seg_lo, int* __restrict__ seg_hi, const int* __restrict__ is_left,
                                                        const Int3* __restrict__ scan, int n, int* __restrict__ bad) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j >= n) return;
  const int lo = seg_lo[j], hi = seg_hi[j];
  if (hi - lo <= 1) {
    for (int a = 0; a < 3; ++a) O.l[a][j] = L.l[a][j];
    return;
  }
  const int mid = kd_mid(lo, hi);
  const Int3 base = scan[lo], here = scan[j];
  for (int a = 0; a < 3; ++a) {
    const int item = L.l[a][j];
    const int lb = here.v[a] - base.v[a];
    const int pos = is_left[item] ? lo + lb : mid + (j - lo - lb);
    if (pos < lo || pos >= hi) { *bad = 1; continue; }   // (cannot happen: every segment holds the same points in all three lists)
    O.l[a][pos] = item;
  }
  seg_lo[j] = j < mid ? lo : mid;
  seg_hi[j] = j < mid ? mid : hi;
}

__global__ __launch_bounds__(BT) void fill_segments_kernel(int* __restrict__ seg_lo, int* __restrict__ seg_hi, int n) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j < n) { seg_lo[j] = 0; seg_hi[j] = n; }
}

// ---- gathers -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void gather_kernel(const double* __restrict__ xyz, const double* __restrict__ nor, const int* __restrict__ order,
                                                    const int* __restrict__ corder, int n, double* __restrict__ spts, int* __restrict__ sidx,
                                                    PointRec* __restrict__ srec, PointRec* __restrict__ crec, int* __restrict__ inv, double* __restrict__ snor) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const int o = order[i];
  const double x = xyz[3 * (size_t)o], y = xyz[3 * (size_t)o + 1], z = xyz[3 * (size_t)o + 2];
  spts[3 * (size_t)i] = x; spts[3 * (size_t)i + 1] = y; spts[3 * (size_t)i + 2] = z;
  sidx[i] = o;
  srec[i] = PointRec{x, y, z, (long long)o};
  inv[o] = i;
  if (snor) { snor[3 * (size_t)i] = nor[3 * (size_t)o]; snor[3 * (size_t)i + 1] = nor[3 * (size_t)o + 1]; snor[3 * (size_t)i + 2] = nor[3 * (size_t)o + 2]; }
  if (crec) {
    const int co = corder[i];
    crec[i] = PointRec{xyz[3 * (size_t)co], xyz[3 * (size_t)co + 1], xyz[3 * (size_t)co + 2], (long long)co};
  }
}

// ---- boxes ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void oct_leaf_kernel(const double* __restrict__ spts, int n, int L8, long long leaves, long long first_leaf, float* __restrict__ oct) {
  const long long j = (long long)blockIdx.x * BT + threadIdx.x;
  if (j >= leaves) return;
  const long long a = j * L8 < n ? j * L8 : n, b = a + L8 < n ? a + L8 : n;
  float bx[8] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.f, 0.f};
  for (long long k = a; k < b; ++k)
    for (int ax = 0; ax < 3; ++ax) { bx[ax] = fmin_first(bx[ax], f32_down(spts[3 * k + ax])); bx[3 + ax] = fmax_first(bx[3 + ax], f32_up(spts[3 * k + ax])); }
  float* o = oct + 8 * (first_leaf + j);
  for (int q = 0; q < 8; ++q) o[q] = bx[q];
}

__global__ __launch_bounds__(BT) void oct_parent_kernel(float* __restrict__ oct, long long first, long long count) {
  const long long t = (long long)blockIdx.x * BT + threadIdx.x;
  if (t >= count) return;
  const long long id = first + t;
  float bx[8] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.f, 0.f};
  for (int ch = 1; ch <= 8; ++ch) {
    const float* cb = oct + 8 * (8 * id + ch);
    for (int ax = 0; ax < 3; ++ax) { bx[ax] = fmin_first(bx[ax], cb[ax]); bx[3 + ax] = fmax_first(bx[3 + ax], cb[3 + ax]); }
  }
  for (int q = 0; q < 8; ++q) oct[8 * id + q] = bx[q];
}

__global__ __launch_bounds__(BT) void wide_leaf_kernel(const double* __restrict__ spts, int n, int cnt, float* __restrict__ b) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j >= cnt) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int e = (j + 1) * LEAF < n ? (j + 1) * LEAF : n;
  for (int k = j * LEAF; k < e; ++k)
    for (int a = 0; a < 3; ++a) { lo[a] = fmin_first(lo[a], f32_down(spts[3 * (size_t)k + a])); hi[a] = fmax_first(hi[a], f32_up(spts[3 * (size_t)k + a])); }
  for (int a = 0; a < 3; ++a) { b[(size_t)a * cnt + j] = lo[a]; b[(size_t)(3 + a) * cnt + j] = hi[a]; }
}

__global__ __launch_bounds__(BT) void wide_up_kernel(const float* __restrict__ p, int pc, int cnt, float* __restrict__ b) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j >= cnt) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int e = (j + 1) * FAN < pc ? (j + 1) * FAN : pc;
  for (int k = j * FAN; k < e; ++k)
    for (int a = 0; a < 3; ++a) { lo[a] = fmin_first(lo[a], p[(size_t)a * pc + k]); hi[a] = fmax_first(hi[a], p[(size_t)(3 + a) * pc + k]); }
  for (int a = 0; a < 3; ++a) { b[(size_t)a * cnt + j] = lo[a]; b[(size_t)(3 + a) * cnt + j] = hi[a]; }
}

// ---- matrix-pipe operands: one workgroup per block of FAN x LEAF points ------------------------------------------------------------------
constexpr int MB = 256;
constexpr int kPerThread = FAN * LEAF / MB;   // consecutive points per thread

// largest s with ldexp(ext, s) <= 127, as build_mfma's floor(log2(127 / ext)) + decrement loop finds it (frexp: ext = m 2^e, 127 = (127/128) 2^7);
// clamped to +-900; 0 when ext is 0 or not finite.  (Where 127 / ext overflows, the host's conversion of an infinite floor yields INT_MIN: -900.)
__device__ __forceinline__ int mf_scale_exp(double ext) {
  if (!(ext > 0.0 && isfinite(ext))) return 0;
  if (!(127.0 / ext <= 1.7976931348623157e308)) return -900;
  int e;
  const double m = frexp(ext, &e);
  const int s = (m <= 0.9921875 ? 7 : 6) - e;
  return s < -900 ? -900 : s > 900 ? 900 : s;
}

__global__ __launch_bounds__(MB) void mfma_block_kernel(const double* __restrict__ spts, int n, int tiles, double cloud_max,
                                                        unsigned short* __restrict__ ops, MfBlock* __restrict__ blk) {
  __shared__ double slo[3][MB], shi[3][MB];
  __shared__ double sc[4];
  __shared__ double sdb[MB], sen[MB];
  const int b = blockIdx.x, t = threadIdx.x;
  const int p0 = b * FAN * LEAF, p1 = min(n, (b + 1) * FAN * LEAF);
  // lo / hi with std::min / std::max's rule (the earlier operand wins a tie: decides the sign of a zero bound, hence of the centre):
  // contiguous chunks per thread, then a tree in which the left operand always holds the earlier points
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int k = p0 + t * kPerThread; k < min(p1, p0 + (t + 1) * kPerThread); ++k)
    for (int a = 0; a < 3; ++a) { lo[a] = dmin_first(lo[a], spts[3 * (size_t)k + a]); hi[a] = dmax_first(hi[a], spts[3 * (size_t)k + a]); }
  for (int a = 0; a < 3; ++a) { slo[a][t] = lo[a]; shi[a][t] = hi[a]; }
  __syncthreads();
  for (int s = 1; s < MB; s <<= 1) {
    if ((t & (2 * s - 1)) == 0)
      for (int a = 0; a < 3; ++a) { slo[a][t] = dmin_first(slo[a][t], slo[a][t + s]); shi[a][t] = dmax_first(shi[a][t], shi[a][t + s]); }
    __syncthreads();
  }
  if (t == 0) {
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
      sc[a] = b_mul(0.5, b_add(slo[a][0], shi[a][0]));
      ext = dmax_first(ext, dmax_first(b_sub(shi[a][0], sc[a]), b_sub(sc[a], slo[a][0])));
    }
    sc[3] = ldexp(1.0, mf_scale_exp(ext));
  }
  __syncthreads();
  const double c[3] = {sc[0], sc[1], sc[2]}, scale = sc[3];
  double db = 0.0, en = 0.0;
  const int t_end = min(tiles, (b + 1) * FAN);
  for (int q = t; q < FAN * LEAF; q += MB) {
    const int tile = b * FAN + q / LEAF, i = q % LEAF;
    if (tile >= t_end) break;
    const int k = tile * LEAF + i;
    unsigned short lo8[8], hi8[8];
    double res, e;
    mf_point(k < n ? spts + 3 * (size_t)k : nullptr, c, scale, lo8, hi8, res, e);
    if (k < n) { en = fmax(en, e); db = fmax(db, res); }   // (non-negative: order-free)
    uint4* o = (uint4*)(ops + ((size_t)tile * 64 + i) * 8);
    uint4 v;
    __builtin_memcpy(&v, lo8, 16); o[0] = v;
    __builtin_memcpy(&v, hi8, 16); o[32] = v;
  }
  sdb[t] = db; sen[t] = en;
  __syncthreads();
  for (int s = MB / 2; s > 0; s >>= 1) {
    if (t < s) { sdb[t] = fmax(sdb[t], sdb[t + s]); sen[t] = fmax(sen[t], sen[t + s]); }
    __syncthreads();
  }
  if (t == 0) {
    MfBlock B;
    B.cx = c[0]; B.cy = c[1]; B.cz = c[2]; B.scale = scale;
    B.db = mf_block_db(sdb[0], cloud_max, c, scale);
    B.en = mf_block_en(sen[0]);
    B.pad0 = B.pad1 = 0.f;
    blk[b] = B;
  }
}

inline unsigned int grid_of(long long n) { return (unsigned int)std::max<long long>(1, (n + BT - 1) / BT); }

// one scratch allocation per build, carved into aligned pieces
struct Carve {
  char* base; size_t off = 0;
  template <typename T> T* take(size_t count) { off = (off + 255) & ~(size_t)255; T* p = (T*)(base + off); off += sizeof(T) * std::max<size_t>(count, 1); return p; }
};

struct Scratch { void* p = nullptr; ~Scratch() { if (p) (void)hipFree(p); } };
struct OwnStream { hipStream_t s = nullptr; ~OwnStream() { if (s) (void)hipStreamDestroy(s); } };

}  // namespace

int device_bounds(hipStream_t stream, const double* d_xyz, int n, DevBounds* out) {
  DevBounds* d_part = nullptr;
  MV_HIP(hipMalloc((void**)&d_part, sizeof(DevBounds) * kBoundsParts));
  Scratch guard; guard.p = d_part;
  const int parts = (int)std::min<long long>(kBoundsParts, grid_of(n));
  hipLaunchKernelGGL(bounds_kernel, dim3(parts), dim3(BT), 0, stream, d_xyz, n, d_part);
  MV_HIP(hipGetLastError());
  std::vector<DevBounds> h(parts);
  MV_HIP(hipMemcpyAsync(h.data(), d_part, sizeof(DevBounds) * parts, hipMemcpyDeviceToHost, stream));
  MV_HIP(hipStreamSynchronize(stream));
  DevBounds b = h[0];
  for (int p = 1; p < parts; ++p) {
    for (int a = 0; a < 3; ++a) { b.lo[a] = std::fmin(b.lo[a], h[p].lo[a]); b.hi[a] = std::fmax(b.hi[a], h[p].hi[a]); }
    b.max_norm = std::fmax(b.max_norm, h[p].max_norm); b.maxabs = std::fmax(b.maxabs, h[p].maxabs); b.nonfinite |= h[p].nonfinite;
  }
  *out = b;
  return MVICP_OK;
}

int build_grid_device(mvicp_ctx* c, FrameDev& f, const DevBounds& bounds, int grid_curve, double grid_target) {
  const auto t0 = std::chrono::steady_clock::now();
  const int n = f.n;
  GridDev& G = f.grid;
  const double* xyz = f.pts;
  OwnStream own;
  MV_HIP(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
  const hipStream_t st = own.s;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  MV_HIP(hipEventCreate(&ev0)); MV_HIP(hipEventCreate(&ev1));
  struct Events { hipEvent_t& a; hipEvent_t& b; ~Events() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } events{ev0, ev1};
  MV_HIP(hipEventRecord(ev0, st));

  const bool split_orders = grid_curve >= 2 && n > 64;
  int set_log2 = 4;
  while ((1ull << set_log2) < 2ull * (unsigned long long)n + 2) ++set_log2;
  const size_t set_size = (size_t)1 << set_log2;

  // rocPRIM's temporary storage: the largest of the sorts and scans below
  size_t sort_bytes = 0, scan_bytes = 0, scan3_bytes = 0;
  MV_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)n, 0, 64, st));
  MV_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (int*)nullptr, (int*)nullptr, 0, (size_t)n, rocprim::plus<int>(), st));
  MV_HIP(rocprim::exclusive_scan(nullptr, scan3_bytes, (Int3*)nullptr, (Int3*)nullptr, Int3{{0, 0, 0}}, (size_t)n, Int3Sum(), st));
  const size_t tmp_bytes = std::max(sort_bytes, std::max(scan_bytes, scan3_bytes));
  const size_t N = (size_t)n;
  const size_t need = 256 * 24 + tmp_bytes + N * (8 * 3 + 4 * 2 + 4 * 4 + 16) + set_size * 8 + (split_orders ? N * (4 * 6 + 4 * 3 + 12 * 2) : 0) + 64;
  Scratch scratch;
  MV_HIP(hipMalloc(&scratch.p, need));
  Carve cv{(char*)scratch.p};
  void* tmp = cv.take<char>(tmp_bytes);
  unsigned long long* key_a = cv.take<unsigned long long>(N);
  unsigned long long* key_b = cv.take<unsigned long long>(N);
  unsigned long long* ckey = cv.take<unsigned long long>(N);
  int* idx_a = cv.take<int>(N);
  int* corder = cv.take<int>(N);
  int* head = cv.take<int>(N);
  int* rid = cv.take<int>(N);
  int* rstart = cv.take<int>(N);
  unsigned int* counters = cv.take<unsigned int>(16);   // [0] occupancy, [1] runs, [2] k-d consistency
  HashEntry* d_runs = cv.take<HashEntry>(N);
  unsigned long long* set = cv.take<unsigned long long>(set_size);
  if (cv.off > need) { set_error("device build: scratch layout overflow"); return MVICP_ERR_INTERNAL; }

  // cell size: the host heuristic over device occupancy counts
  HostGrid g;
  unsigned int h_count = 0;
  const int occ_status = choose_grid(g, n, bounds.lo, bounds.hi, grid_target, [&](const HostGrid& gg) -> long long {
    if (hipMemsetAsync(set, 0xFF, set_size * 8, st) != hipSuccess || hipMemsetAsync(counters, 0, sizeof(unsigned int), st) != hipSuccess) return MVICP_ERR_HIP;
    hipLaunchKernelGGL(occupancy_kernel, dim3(grid_of(n)), dim3(BT), 0, st, xyz, n, gg, set, (unsigned int)(set_size - 1), 64 - set_log2, counters);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_count, counters, sizeof(unsigned int), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return MVICP_ERR_HIP;
    return (long long)h_count;
  });
  if (occ_status < 0) { set_error("device build: occupancy count failed"); return occ_status; }

  // cell order: stable radix sort of (curve key, index)
  const int hbits = curve_bits(g);
  hipLaunchKernelGGL(curve_keys_kernel, dim3(grid_of(n)), dim3(BT), 0, st, xyz, n, g, grid_curve, hbits, key_a, ckey, idx_a);
  MV_HIP(hipGetLastError());
  size_t tb = 0;
  MV_HIP(rocprim::radix_sort_pairs(nullptr, tb, key_a, key_b, idx_a, corder, N, 0, 3 * hbits, st));
  if (tb > tmp_bytes) { set_error("device build: sort storage %zu > %zu", tb, tmp_bytes); return MVICP_ERR_INTERNAL; }
  MV_HIP(rocprim::radix_sort_pairs(tmp, tb, key_a, key_b, idx_a, corder, N, 0, 3 * hbits, st));
  hipLaunchKernelGGL(run_heads_kernel, dim3(grid_of(n)), dim3(BT), 0, st, ckey, corder, n, head);
  MV_HIP(hipGetLastError());
  tb = tmp_bytes;
  MV_HIP(rocprim::exclusive_scan(tmp, tb, head, rid, 0, N, rocprim::plus<int>(), st));
  hipLaunchKernelGGL(run_starts_kernel, dim3(grid_of(n)), dim3(BT), 0, st, head, rid, n, rstart, (int*)counters + 1);
  MV_HIP(hipGetLastError());
  hipLaunchKernelGGL(run_list_kernel, dim3(grid_of(n)), dim3(BT), 0, st, ckey, corder, rstart, (const int*)counters + 1, n, d_runs);
  MV_HIP(hipGetLastError());
  int R = 0;
  MV_HIP(hipMemcpyAsync(&R, counters + 1, sizeof(int), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (R <= 0 || R > n) { set_error("device build: bad run count %d", R); return MVICP_ERR_INTERNAL; }
  std::vector<HashEntry> runs((size_t)R);
  MV_HIP(hipMemcpyAsync(runs.data(), d_runs, sizeof(HashEntry) * (size_t)R, hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));

  // canonical order
  const int* order = corder;
  if (split_orders) {
    int* L[2][3];
    for (int p = 0; p < 2; ++p)
      for (int a = 0; a < 3; ++a) L[p][a] = cv.take<int>(N);
    int* is_left = cv.take<int>(N);
    int* seg_lo = cv.take<int>(N);
    int* seg_hi = cv.take<int>(N);
    Int3* flags = cv.take<Int3>(N);
    Int3* scan = cv.take<Int3>(N);
    if (cv.off > need) { set_error("device build: scratch layout overflow"); return MVICP_ERR_INTERNAL; }
    for (int a = 0; a < 3; ++a) {
      hipLaunchKernelGGL(coord_keys_kernel, dim3(grid_of(n)), dim3(BT), 0, st, xyz, n, a, key_a, idx_a);
      MV_HIP(hipGetLastError());
      tb = tmp_bytes;
      MV_HIP(rocprim::radix_sort_pairs(tmp, tb, key_a, key_b, idx_a, L[0][a], N, 0, 64, st));
    }
    hipLaunchKernelGGL(fill_segments_kernel, dim3(grid_of(n)), dim3(BT), 0, st, seg_lo, seg_hi, n);
    MV_HIP(hipGetLastError());
    MV_HIP(hipMemsetAsync(counters + 2, 0, sizeof(unsigned int), st));
    // levels: the largest segment of a level is the left child of the previous level's largest
    int levels = 0;
    for (long long m = n; m > 1; ++levels) {
      const long long units = m > 32 ? (m + 31) / 32 : m, unit = m > 32 ? 32 : 1;
      long long left = 1;
      while (left * 2 < units) left *= 2;
      m = left * unit;
    }
    int cur = 0;
    for (int lv = 0; lv < levels; ++lv) {
      const Lists in{{L[cur][0], L[cur][1], L[cur][2]}};
      const OutLists out{{L[1 - cur][0], L[1 - cur][1], L[1 - cur][2]}};
      hipLaunchKernelGGL(kd_flag_kernel, dim3(grid_of(n)), dim3(BT), 0, st, in, xyz, seg_lo, seg_hi, n, is_left);
      hipLaunchKernelGGL(kd_count_kernel, dim3(grid_of(n)), dim3(BT), 0, st, in, seg_lo, seg_hi, is_left, n, flags);
      MV_HIP(hipGetLastError());
      tb = tmp_bytes;
      MV_HIP(rocprim::exclusive_scan(tmp, tb, flags, scan, Int3{{0, 0, 0}}, N, Int3Sum(), st));
      hipLaunchKernelGGL(kd_scatter_kernel, dim3(grid_of(n)), dim3(BT), 0, st, in, out, seg_lo, seg_hi, is_left, scan, n, (int*)counters + 2);
      MV_HIP(hipGetLastError());
      cur = 1 - cur;
    }
    order = L[cur][0];
  }

  // gathers
  MV_HIP(hipMalloc((void**)&G.spts, sizeof(double) * 3 * N));
  MV_HIP(hipMalloc((void**)&G.sidx, sizeof(int) * N));
  MV_HIP(hipMalloc((void**)&G.srec, sizeof(PointRec) * N));
  G.crec = G.srec;
  if (split_orders) MV_HIP(hipMalloc((void**)&G.crec, sizeof(PointRec) * N));
  MV_HIP(hipMalloc((void**)&G.inv, sizeof(int) * N));
  if (f.nor) MV_HIP(hipMalloc((void**)&G.snor, sizeof(double) * 3 * N));
  hipLaunchKernelGGL(gather_kernel, dim3(grid_of(n)), dim3(BT), 0, st, xyz, f.nor, order, corder, n, G.spts, G.sidx, (PointRec*)G.srec,
                     split_orders ? (PointRec*)G.crec : (PointRec*)nullptr, G.inv, G.snor);
  MV_HIP(hipGetLastError());

  // hash table + brick map from the run list, on the host exactly as the host build makes them
  std::vector<HashEntry> table;
  unsigned int mask = 0; int shift = 0;
  hash_runs(runs, table, mask, shift);
  const unsigned int tsize = mask + 1;
  MV_HIP(hipMalloc((void**)&G.table, sizeof(HashEntry) * (size_t)tsize));
  MV_HIP(hipMemcpyAsync(G.table, table.data(), sizeof(HashEntry) * (size_t)tsize, hipMemcpyHostToDevice, st));
  std::vector<BrickEntry> bricks;
  std::vector<uint2> celltab;
  if (brick_map(runs, g, n, split_orders, bricks, celltab, G.bdims)) {
    MV_HIP(hipMalloc((void**)&G.bricks, sizeof(BrickEntry) * bricks.size()));
    MV_HIP(hipMemcpyAsync(G.bricks, bricks.data(), sizeof(BrickEntry) * bricks.size(), hipMemcpyHostToDevice, st));
    MV_HIP(hipMalloc((void**)&G.celltab, sizeof(uint2) * std::max<size_t>(celltab.size(), 1)));
    if (!celltab.empty()) MV_HIP(hipMemcpyAsync(G.celltab, celltab.data(), sizeof(uint2) * celltab.size(), hipMemcpyHostToDevice, st));
    G.celltab_bytes = sizeof(uint2) * celltab.size();
  }

  // 8-ary box tree
  int D8 = 0, L8 = 8;
  oct_shape(n, D8, L8);
  const long long leaves8 = 1ll << (3 * D8), first_leaf8 = (leaves8 - 1) / 7, nodes8 = first_leaf8 + leaves8;
  MV_HIP(hipMalloc((void**)&G.oct, sizeof(float) * 8 * (size_t)nodes8));
  hipLaunchKernelGGL(oct_leaf_kernel, dim3(grid_of(leaves8)), dim3(BT), 0, st, G.spts, n, L8, leaves8, first_leaf8, G.oct);
  MV_HIP(hipGetLastError());
  for (int d = D8 - 1; d >= 0; --d) {
    const long long first = ((1ll << (3 * d)) - 1) / 7, count = 1ll << (3 * d);
    hipLaunchKernelGGL(oct_parent_kernel, dim3(grid_of(count)), dim3(BT), 0, st, G.oct, first, count);
    MV_HIP(hipGetLastError());
  }
  G.oct_leaf = L8; G.oct_first_leaf = first_leaf8;

  // 64-wide hierarchy (build_wide's level counts and limit)
  {
    std::vector<int> cnts;
    int cnt = (n + LEAF - 1) / LEAF;
    cnts.push_back(cnt);
    while (cnt > FAN) {
      cnt = (cnt + FAN - 1) / FAN;
      if (cnts.size() >= 5) { set_error("cloud too large for the 64-wide hierarchy"); return MVICP_ERR_ARG; }
      cnts.push_back(cnt);
    }
    size_t total = 0;
    for (size_t l = 0; l < cnts.size(); ++l) { G.wide_off[l] = (long long)total; G.wide_cnt[l] = cnts[l]; total += 6 * (size_t)cnts[l]; }
    G.wide_levels = (int)cnts.size();
    MV_HIP(hipMalloc((void**)&G.wide, sizeof(float) * std::max<size_t>(total, 1)));
    hipLaunchKernelGGL(wide_leaf_kernel, dim3(grid_of(cnts[0])), dim3(BT), 0, st, G.spts, n, cnts[0], G.wide);
    MV_HIP(hipGetLastError());
    for (size_t l = 1; l < cnts.size(); ++l) {
      hipLaunchKernelGGL(wide_up_kernel, dim3(grid_of(cnts[l])), dim3(BT), 0, st, G.wide + G.wide_off[l - 1], cnts[l - 1], cnts[l], G.wide + G.wide_off[l]);
      MV_HIP(hipGetLastError());
    }
    G.maxabs = bounds.maxabs;
  }

  // matrix-pipe operands
  {
    const int tiles = (n + LEAF - 1) / LEAF, blocks = (tiles + FAN - 1) / FAN;
    const size_t ops_bytes = (size_t)std::max(tiles, 1) * 64 * 8 * sizeof(unsigned short);
    MV_HIP(hipMalloc(&G.mf_ops, ops_bytes));
    MV_HIP(hipMemsetAsync(G.mf_ops, 0, ops_bytes, st));
    MV_HIP(hipMalloc(&G.mf_blk, sizeof(MfBlock) * (size_t)std::max(blocks, 1)));
    hipLaunchKernelGGL(mfma_block_kernel, dim3(blocks), dim3(MB), 0, st, G.spts, n, tiles, bounds.maxabs, (unsigned short*)G.mf_ops, (MfBlock*)G.mf_blk);
    MV_HIP(hipGetLastError());
  }

  G.dims[0] = g.d[0]; G.dims[1] = g.d[1]; G.dims[2] = g.d[2];
  G.origin[0] = g.o[0]; G.origin[1] = g.o[1]; G.origin[2] = g.o[2];
  G.cell = g.h; G.inv_cell = g.inv_h;
  G.n_cells = R;
  G.table_mask = mask; G.table_shift = shift;
  G.struct_bytes = sizeof(HashEntry) * (double)tsize + sizeof(float) * 8.0 * nodes8;

  // host copies of the order
  MV_HIP(hipEventRecord(ev1, st));
  G.h_order.resize(N); G.h_inv.resize(N);
  unsigned int bad = 0;
  MV_HIP(hipMemcpyAsync(G.h_order.data(), G.sidx, sizeof(int) * N, hipMemcpyDeviceToHost, st));
  MV_HIP(hipMemcpyAsync(G.h_inv.data(), G.inv, sizeof(int) * N, hipMemcpyDeviceToHost, st));
  MV_HIP(hipMemcpyAsync(&bad, counters + 2, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (split_orders && bad) { set_error("device build: inconsistent k-d partition"); return MVICP_ERR_INTERNAL; }
  float dev_ms = 0.f;
  MV_HIP(hipEventElapsedTime(&dev_ms, ev0, ev1));
  f.build_ms[0] = bounds.wall_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  f.build_ms[1] = dev_ms;
  f.has_grid = true;
  return MVICP_OK;
}

}  // namespace mvicp
