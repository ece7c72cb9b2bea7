// ISS keypoints (mvicp_iss_keypoints): per point of the stored cloud the eigenvalues l1 >= l2 >= l3 of the covariance of its neighbourhood
// within salient_radius, the saliency l3 of the points that pass the two ratio tests, and the points no neighbour within non_max_radius
// beats.  The result is a pure function of the stored bytes (the contract is stated in include/mvicp.h; tests/issref.py is its numpy
// form).  DESIGN.md §3.13.
//
// Passes, all on the context's stream, no host wait before the last one:
//   1  moments  one lane per point in hash-CELL order (GridDev::crec): traverse() of knn_traverse.h (stop rule B2 <= m m)
//               whose offer adds the neighbour's count and nine integer sums in registers -- g = floor((p_j - p_i) 2^q) fits an int, so a
//               product is one 32 x 32 -> 64 multiply-add, and integer sums do not depend on the visiting order: no row is stored and
//               nothing is sorted.  Then, in the same lane, D = c S - m m^T, C = D / c^2, six Jacobi sweeps and the tests; saliency and
//               count go to the point's ORIGINAL index.
//   2  nms      the same traversal at non_max_radius; offer reads the neighbour's saliency by its original index -> flag, count
//   3  compact  select_rows (row_select.h): the flagged indices, ascending, and their stored rows (the fetch only copies)
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "jacobi3.h"
#include "knn_traverse.h"
#include "nn_metric.h"
#include "row_select.h"

namespace mvicp {

namespace {

constexpr int NT = 128;          // lanes per workgroup of the two traversal passes
constexpr int kIssCap = 1024;    // neighbours of a salient row; more: MVICP_ERR_ARG
constexpr int kSweeps = 6;
constexpr unsigned int kFlagTooMany = 1u;

struct IssCtl { unsigned int flags, pad; };
constexpr size_t kTreeOffset = 64, kHeadBytes = 256;   // the box-tree view lives in the control block (knn.hip: TreeView)

struct IssJob {
  GridView g;
  const TreeView* tree;   // null: no box tree
  double B2;              // sqrt(d2) < radius  <=>  d2 < B2
  double scale, unscale;  // 2^q, 2^-2q
  double g21, g32;
  int min_nb, pad;
  double* sal;            // n, original order
  int* cnt;               // n, original order: this pass's count
  int* flag;              // n, original order (pass 2)
  IssCtl* ctl;
};

__device__ __forceinline__ int scaled_floor(double pj, double pi, double scale) { return (int)floor(__dmul_rn(__dsub_rn(pj, pi), scale)); }

__global__ __launch_bounds__(NT) void iss_moments_kernel(IssJob job) {
  const int i = blockIdx.x * NT + threadIdx.x;   // position in cell order
  if (i >= job.g.n) return;
  const PointRec me = job.g.crec[i];
  const double B2 = job.B2, scale = job.scale;
  int c = 0;
  long long m0 = 0, m1 = 0, m2 = 0, s00 = 0, s01 = 0, s02 = 0, s11 = 0, s12 = 0, s22 = 0;
  auto offer = [&](double d, const PointRec* p) {
    if (!(d < B2)) return;
    if (++c > kIssCap) return;   // (reported below; the sums of such a row are not used, and they stay below 2^62)
    const int g0 = scaled_floor(p->x, me.x, scale), g1 = scaled_floor(p->y, me.y, scale), g2 = scaled_floor(p->z, me.z, scale);
    m0 += g0; m1 += g1; m2 += g2;
    s00 += (long long)g0 * g0; s01 += (long long)g0 * g1; s02 += (long long)g0 * g2;
    s11 += (long long)g1 * g1; s12 += (long long)g1 * g2; s22 += (long long)g2 * g2;
  };
  auto reset = [&]() { c = 0; m0 = m1 = m2 = s00 = s01 = s02 = s11 = s12 = s22 = 0; };
  auto stop = [&](double mm) { return B2 <= mm; };
  auto open = [&](double lb) { return lb < B2; };
  auto seed = [&](double) {};
  traverse(job.g, job.tree, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);

  double sal = 0.0;
  if (c > kIssCap) atomicOr(&job.ctl->flags, kFlagTooMany);
  else if (c >= job.min_nb) {   // (c >= 1: the point itself)
    const long long cc = c;
    const double den = __ll2double_rn(cc * cc);   // <= 2^20: exact
    const double c00 = __ddiv_rn(__ll2double_rn(cc * s00 - m0 * m0), den), c01 = __ddiv_rn(__ll2double_rn(cc * s01 - m0 * m1), den);
    const double c02 = __ddiv_rn(__ll2double_rn(cc * s02 - m0 * m2), den), c11 = __ddiv_rn(__ll2double_rn(cc * s11 - m1 * m1), den);
    const double c12 = __ddiv_rn(__ll2double_rn(cc * s12 - m1 * m2), den), c22 = __ddiv_rn(__ll2double_rn(cc * s22 - m2 * m2), den);
    // the diagonal after kSweeps sweeps of jacobi3.h: no exit test, no vectors
    jacobi3::M33 A = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) jacobi3::sweep(A);
    const double a = A.m00, b = A.m11, e = A.m22;
    const double l1 = fmax(fmax(a, b), e), l3 = fmin(fmin(a, b), e);
    const double l2 = fmax(fmin(a, b), fmin(fmax(a, b), e));   // the median of three
    if (l2 < __dmul_rn(job.g21, l1) && l3 < __dmul_rn(job.g32, l2) && l3 > 0.0) sal = __dmul_rn(l3, job.unscale);
  }
  job.sal[me.idx] = sal;
  job.cnt[me.idx] = c;
}

__global__ __launch_bounds__(NT) void iss_nms_kernel(IssJob job) {
  const int i = blockIdx.x * NT + threadIdx.x;   // position in cell order
  if (i >= job.g.n) return;
  const PointRec me = job.g.crec[i];
  const double B2 = job.B2;
  const double mine = job.sal[me.idx];
  const double* __restrict__ sal = job.sal;
  int c = 0;
  bool beaten = false;
  auto offer = [&](double d, const PointRec* p) {
    if (!(d < B2)) return;
    ++c;
    const double s = sal[p->idx];
    beaten = beaten || s > mine || (s == mine && p->idx < me.idx);
  };
  auto reset = [&]() { c = 0; beaten = false; };
  auto stop = [&](double mm) { return B2 <= mm; };
  auto open = [&](double lb) { return lb < B2; };
  auto seed = [&](double) {};
  traverse(job.g, job.tree, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);
  job.cnt[me.idx] = c;
  job.flag[me.idx] = (mine > 0.0 && c >= job.min_nb && !beaten) ? 1 : 0;
}

}  // namespace

long long iss_keypoints(mvicp_ctx* c, const FrameDev& f, double B2_salient, double B2_nms, int q, double gamma21, double gamma32, int min_neighbors) {
  c->iss.n = -1; c->iss.sel.drop();   // (the last result ends here; a failed call leaves none behind)
  const int n = f.n;
  if (n > 0 && !f.has_grid) { set_error("the keypoints need the per-cloud hash structure%s%s", f.build_error.empty() ? "" : ": ", f.build_error.c_str()); return MVICP_ERR_STATE; }
  const auto select = [&]() { return select_rows(c, c->iss.sel, f, "iss keypoints", "iss_compact", 12.0, nullptr, 0); };
  if (n == 0) { c->iss.n = 0; return select(); }   // (an empty selection: no launch, no wait)
  hipStream_t st = c->stream;
  const size_t N = (size_t)n;

  // the per-point results in one arena: [control | saliency | cnt_salient | cnt_nms]
  const size_t o_sal = kHeadBytes, o_cs = o_sal + align256(8 * N), o_cn = o_cs + align256(4 * N);
  MV_CHECK(c->iss.dev.reserve(o_cn + align256(4 * N)));
  MV_CHECK(c->iss.pin.reserve(256));
  MV_CHECK(c->iss.sel.reserve(n, false, st));
  char* D = c->iss.dev.p;
  IssCtl* d_ctl = reinterpret_cast<IssCtl*>(D);
  IssCtl* h_ctl = reinterpret_cast<IssCtl*>(c->iss.pin.p);
  c->iss.sal = reinterpret_cast<double*>(D + o_sal); c->iss.cnt_s = reinterpret_cast<int*>(D + o_cs); c->iss.cnt_n = reinterpret_cast<int*>(D + o_cn);
  MV_HIP(hipMemsetAsync(d_ctl, 0, sizeof(IssCtl), st));

  IssJob j;
  std::memset(&j, 0, sizeof(j));
  const GridDev& g = f.grid;
  fill_grid_view(&j.g, g, n);
  // words 0 .. 1 of the pinned block receive the control block, the tree view is staged behind them
  MV_CHECK(stage_tree_view(g, c->iss.pin.p + kTreeOffset, D + kTreeOffset, st, &j.tree));
  j.scale = std::ldexp(1.0, q); j.unscale = std::ldexp(1.0, -2 * q);
  j.g21 = gamma21; j.g32 = gamma32; j.min_nb = min_neighbors;
  j.sal = c->iss.sal; j.flag = c->iss.sel.flag; j.ctl = d_ctl;
  {
    ProfScope ps(c, "iss_moments", 44.0 * n);
    j.B2 = B2_salient; j.cnt = c->iss.cnt_s;
    hipLaunchKernelGGL(iss_moments_kernel, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
    MV_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "iss_nms", 48.0 * n);
    j.B2 = B2_nms; j.cnt = c->iss.cnt_n;
    hipLaunchKernelGGL(iss_nms_kernel, dim3(grid_of(n, NT)), dim3(NT), 0, st, j);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(IssCtl), hipMemcpyDeviceToHost, st));   // (read after the selection's wait)
  const long long keys = select();
  if (keys < 0) return keys;
  if (h_ctl->flags & kFlagTooMany) {
    c->iss.sel.drop();
    set_error("iss keypoints: a point has more than %d neighbours within the salient radius (smaller radius?)", kIssCap);
    return MVICP_ERR_ARG;
  }
  c->iss.n = n;
  return keys;
}

}  // namespace mvicp
