// Statistical and radius outlier removal (mvicp_outlier_filter): per point the k+1 smallest squared distances to the points of its own
// cloud (itself included), from them the k-th distance and the mean distance to the k nearest, and the two classic rules on top.  The
// result is a pure function of the stored cloud, bit for bit (the contract is stated in include/mvicp.h; tests/outlierref.py is its
// numpy form).  DESIGN.md §3.8.
//
// Passes, all on the context's stream:
//   1  knn      one lane per point in hash-CELL order (GridDev::crec): traverse() of knn_traverse.h without a box tree, stopping once
//               the k+1-th value lies inside the scanned block's faces, VALUES ONLY: no index, no tie order, no PCA.  Writes kd2 and
//               mdist in original order; one atomic max per wave on the bit pattern of mdist (>= 0).
//      -- host wait (statistical rule only): mmax; the host chooses q_exp --
//   2  sum      M = floor(mdist 2^q_exp) < 2^31; S1 = sum M and the two 32-bit halves of M^2 summed apart (each sum < 2^63 for
//               n < 2^31): wave reduction, then three 64-bit integer atomics per workgroup.  Integer sums: order-independent.
//      -- host wait: the sums; T = mvicp_outlier_threshold --
//   3  flag     keep = ((double)M <= T) and (sqrt(kd2) < radius), each rule only when it is on
//   4  compact  select_rows (row_select.h): the flagged rows at their rank, one host wait for the number kept
// What the knn kernel keeps to itself next to the other users of traverse() (this kernel is the whole feature):
//   * the list capacity is a template parameter (9 / 17 / 33 doubles per lane, one LDS column per lane): 9 / 17 / 33 KiB per 128-lane
//     workgroup, so k <= 8 still runs at the 32-waves-per-CU cap, k <= 16 at 18 waves and only k > 16 at 8 (160 KiB of LDS per CU);
//   * the current k+1-th value stays in a register: a candidate that cannot enter the list costs one comparison and no LDS access
//     (after the first cell nearly every candidate);
//   * the list holds values only, so offer ignores the record.
// Consecutive cell-order lanes read the same few cells, so the candidate loads of a wave are mostly one address (a broadcast from L1).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "knn_traverse.h"
#include "nn_metric.h"
#include "row_select.h"

namespace mvicp {

namespace {

constexpr int NT = 128;   // lanes per workgroup of the knn kernel
constexpr int VT = 256;   // of the streaming passes

struct KnnJob {
  GridView g;
  int k;
  double* mdist; double* kd2;    // n each, original order
  unsigned long long* mmax;      // bit pattern of the largest mdist
};

struct OutCtl { unsigned long long mmax, s1, s2lo, s2hi; };

template <int KCAP>
__global__ __launch_bounds__(NT) void outlier_knn_kernel(KnnJob job) {
  // the lane's k+1 smallest values so far, ascending, +inf where there is none yet: one LDS column per lane (consecutive lanes,
  // consecutive 8-byte words: conflict-free), indexed at run time by the insertion
  __shared__ double s_d[KCAP][NT];
#define LD(t) s_d[t][threadIdx.x]
  const int i = blockIdx.x * NT + threadIdx.x;   // position in cell order
  const bool active = i < job.g.n;
  double md = 0.0;
  if (active) {
    const PointRec me = job.g.crec[i];
    const int L = job.k + 1;
    double worst = INFINITY;   // = LD(L - 1)
    auto reset = [&]() {
      for (int t = 0; t < L; ++t) LD(t) = INFINITY;
      worst = INFINITY;
    };
    auto offer = [&](double d, const PointRec*) {
      if (!(d < worst)) return;   // (an equal value changes nothing: only the values enter)
      int pos = L - 1;
      while (pos > 0) {
        const double e = LD(pos - 1);
        if (!(e > d)) break;
        LD(pos) = e;
        --pos;
      }
      LD(pos) = d;
      worst = LD(L - 1);
    };
    auto stop = [&](double m2) { return worst < m2; };   // (implies a full list: +inf is not below it)
    auto open = [](double) { return true; };
    auto seed = [](double) {};
    reset();
    traverse(job.g, nullptr, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);
    double s = 0.0;
    for (int t = 1; t < L; ++t) s = __dadd_rn(s, __dsqrt_rn(LD(t)));
    md = __ddiv_rn(s, (double)job.k);
    job.kd2[me.idx] = worst;
    job.mdist[me.idx] = md;
  }
#undef LD
  unsigned long long b = (unsigned long long)__double_as_longlong(md);   // md >= +0: the bit patterns order like the values
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { const unsigned long long o = __shfl_xor(b, x, 64); b = o > b ? o : b; }
  if ((threadIdx.x & 63) == 0 && b != 0ull) atomicMax(job.mmax, b);
}

__device__ __forceinline__ unsigned long long quantise(double md, int q) { return (unsigned long long)floor(ldexp(md, q)); }

__global__ __launch_bounds__(VT) void outlier_sum_kernel(const double* __restrict__ mdist, int n, int q, OutCtl* __restrict__ ctl) {
  __shared__ unsigned long long s_p[VT / 64][3];
  const int i = blockIdx.x * VT + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long M = i < n ? quantise(mdist[i], q) : 0ull, M2 = M * M;   // M < 2^31
  unsigned long long v[3] = {M, M2 & 0xffffffffull, M2 >> 32};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) v[a] += __shfl_xor(v[a], x, 64);
  if (lane == 0)
    for (int a = 0; a < 3; ++a) s_p[wave][a] = v[a];
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    unsigned long long t = s_p[0][a];
    for (int w = 1; w < VT / 64; ++w) t += s_p[w][a];
    if (t) atomicAdd(a == 0 ? &ctl->s1 : a == 1 ? &ctl->s2lo : &ctl->s2hi, t);
  }
}

__global__ __launch_bounds__(VT) void outlier_flag_kernel(const double* __restrict__ mdist, const double* __restrict__ kd2, int n, int stat, int q, double T,
                                                          int rad, double radius, int* __restrict__ flag) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  bool keep = true;
  if (stat) keep = (double)quantise(mdist[i], q) <= T;
  if (rad) keep = keep && __dsqrt_rn(kd2[i]) < radius;
  flag[i] = keep ? 1 : 0;
}

}  // namespace

long long outlier_filter(mvicp_ctx* c, const FrameDev& f, int k, double std_ratio, double radius, mvicp_outlier_stats* stats) {
  c->out.n = -1; c->out.sel.drop();   // (the last result ends here; a failed call leaves none behind)
  mvicp_outlier_stats S;
  std::memset(&S, 0, sizeof(S));
  S.n = f.n; S.has_normals = f.nor ? 1 : 0;
  const auto select = [&]() { return select_rows(c, c->out.sel, f, "outlier filter", "outlier_compact", f.nor ? 108.0 : 60.0, nullptr, 0); };
  if (f.n == 0) { c->out.n = 0; if (stats) *stats = S; return select(); }   // (an empty selection: no launch, no wait)
  if (!f.has_grid) { set_error("the outlier filter needs the per-cloud hash structure"); return MVICP_ERR_STATE; }
  const int n = f.n;
  const size_t NN = (size_t)n;
  const bool stat_on = std_ratio >= 0.0, rad_on = radius > 0.0;
  hipStream_t st = c->stream;

  // one arena: [control | mdist | kd2]; the per-point results are views into it
  const size_t off_md = 256, off_kd = off_md + align256(8 * NN);
  MV_CHECK(c->out.dev.reserve(off_kd + align256(8 * NN)));
  MV_CHECK(c->out.pin.reserve(256));
  MV_CHECK(c->out.sel.reserve(n, false, st));
  char* D = c->out.dev.p;
  OutCtl* d_ctl = reinterpret_cast<OutCtl*>(D);
  OutCtl* h_ctl = reinterpret_cast<OutCtl*>(c->out.pin.p);
  c->out.mdist = reinterpret_cast<double*>(D + off_md); c->out.kd2 = reinterpret_cast<double*>(D + off_kd);

  MV_HIP(hipMemsetAsync(d_ctl, 0, sizeof(OutCtl), st));
  KnnJob j;
  fill_grid_view(&j.g, f.grid, n);
  j.k = k; j.mdist = c->out.mdist; j.kd2 = c->out.kd2; j.mmax = &d_ctl->mmax;
  {
    ProfScope ps(c, "outlier_knn", 0.0);
    if (k <= 8) hipLaunchKernelGGL(outlier_knn_kernel<9>, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
    else if (k <= 16) hipLaunchKernelGGL(outlier_knn_kernel<17>, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
    else hipLaunchKernelGGL(outlier_knn_kernel<33>, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
  }
  MV_HIP(hipGetLastError());

  int stat = 0, q = 0;
  double T = 0.0;
  if (stat_on) {
    MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(OutCtl), hipMemcpyDeviceToHost, st));
    MV_HIP(hipStreamSynchronize(st));
    double mmax;
    std::memcpy(&mmax, &h_ctl->mmax, 8);
    if (!std::isfinite(mmax)) { set_error("outlier filter: a neighbour distance is not finite (coordinates too large)"); return MVICP_ERR_ARG; }
    if (mmax > 0.0) {
      int ex = 0;
      (void)std::frexp(mmax, &ex);   // mmax = m 2^ex, m in [0.5, 1): mmax 2^(31 - ex) in [2^30, 2^31)
      q = 31 - ex; stat = 1;
      {
        ProfScope ps(c, "outlier_sum", 8.0 * n);
        hipLaunchKernelGGL(outlier_sum_kernel, dim3(grid_of(n, VT)), dim3(VT), 0, st, c->out.mdist, n, q, d_ctl);
      }
      MV_HIP(hipGetLastError());
      MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(OutCtl), hipMemcpyDeviceToHost, st));
      MV_HIP(hipStreamSynchronize(st));
      const unsigned __int128 s2 = ((unsigned __int128)h_ctl->s2hi << 32) + h_ctl->s2lo;
      S.q_exp = q; S.s1 = h_ctl->s1; S.s2_hi = (unsigned long long)(s2 >> 64); S.s2_lo = (unsigned long long)s2;
      MV_CHECK(mvicp_outlier_threshold(n, S.s1, S.s2_hi, S.s2_lo, std_ratio, &T));
      S.T = T; S.threshold = std::ldexp(T, -q);
    }
  }
  {
    ProfScope ps(c, "outlier_flag", 20.0 * n);
    hipLaunchKernelGGL(outlier_flag_kernel, dim3(grid_of(n, VT)), dim3(VT), 0, st, c->out.mdist, c->out.kd2, n, stat, q, T, rad_on ? 1 : 0, radius, c->out.sel.flag);
  }
  MV_HIP(hipGetLastError());
  const long long kept = select();
  if (kept < 0) return kept;
  S.kept = kept;
  if (stats) *stats = S;
  c->out.n = n;
  return kept;
}

}  // namespace mvicp
