// Exact k-nearest / radius neighbour search for arbitrary queries (mvicp_knn_search): per query the candidates of the stored cloud in the
// order (dist2 ascending, ORIGINAL index ascending), the first k of them (k mode, dense rows) or all of them within the radius (all mode,
// CSR).  The result is a pure function of the stored cloud and the queries, bit for bit (the contract is stated in include/mvicp.h;
// tests/knnref.py is its numpy form).  DESIGN.md §3.9.
//
// Passes, all on the context's stream:
//   k mode    1  key     (query mode, option "knn_order") clamped home cell of every query -> linear cell key; rocprim radix sort of (key, query id)
//             2  search  one lane per query in that order (self mode: one lane per point in hash-CELL order, GridDev::crec, nothing to sort):
//                        traverse() of knn_traverse.h with a list of (d2, index) entries; rows go to the query's own position
//   all mode  1  key     as above
//             2  count   the same traversal, counting the points with dist2 < B2; exits on B2 <= m m only
//                -- rocprim exclusive scan of the counts = off; host wait: the total --
//             3  fill    the same traversal again, the candidates of row i stored from off[i] on in visiting order
//             4  order   one wave per row: every entry's rank under (d2, index) by counting, stored at its rank (the pairs are distinct, so the
//                        ranks are a permutation; no sort stability is asked of anything).  O(len^2 / 64) per row: rows of thousands are correct, not fast.
// What the search kernel shares with outlier_knn_kernel: the worst entry in registers (a candidate that cannot enter costs one comparison
// and no LDS access).  The SHELL scan when the block grows (an entry is a real point and stays valid), the scan of the cloud itself once
// the block exceeds 2 n cells (the last resort; a query in empty space goes to the box tree first), the face test for queries outside the
// grid and the box-tree walk are traverse()'s.  This kernel's own: entries carry the original index and the comparator is the contract's
// order, so a candidate with d == worst and a lower index DOES enter; the radius exit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "knn_traverse.h"
#include "nn_metric.h"

namespace mvicp {

namespace {

constexpr int VT = 256;   // lanes per workgroup of the streaming passes
constexpr unsigned int kFlagNonFinite = 1u, kFlagOverflow = 2u;

// where the search kernel puts its rows; read once, after the search, for the same reason
struct RowsView { int* cnt; int* idx; double* d2; };

struct KnnCtl { unsigned long long total; unsigned int flags, pad; };
constexpr size_t kTreeOffset = 64, kRowsOffset = 128;   // of the two views in the control block's 256 bytes

struct KnnJob {
  GridView g;
  const double* q;      // m x 3 queries, or null: self mode (lane i = cell-order position i, row = that point's original index)
  const int* order;     // query mode: lane i answers query order[i] (null: query i)
  const TreeView* tree; // null: no box tree
  int m, k;
  int rad_on; double B2;
  const RowsView* rows;                       // k mode: cnt (m), idx and d2 (m x k)
  int* cnt;                                   // all mode: m
  long long* cnt64; const long long* off;     // all mode: the counts once more as the scan's input (m + 1, the last one 0); the row offsets
  int* eidx; double* ed2;                     // all mode, fill: the entries in visiting order
  KnnCtl* ctl;
};

// lane -> (row, query); false: nothing to do (beyond the end, or a non-finite query, which is flagged)
__device__ __forceinline__ bool lane_query(const KnnJob& job, int i, long long* row, double* qx, double* qy, double* qz) {
  if (i >= job.m) return false;
  if (!job.q) {
    const PointRec me = job.g.crec[i];
    *row = me.idx; *qx = me.x; *qy = me.y; *qz = me.z;
    return true;   // (stored points are finite: mvicp_set_frame checks them)
  }
  const long long r = job.order ? job.order[i] : i;
  const double* q = job.q + 3 * (size_t)r;
  *row = r; *qx = q[0]; *qy = q[1]; *qz = q[2];
  if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2])) return true;
  atomicOr(&job.ctl->flags, kFlagNonFinite);
  return false;
}

__device__ __forceinline__ void add_total(const KnnJob& job, int c) {
  unsigned long long t = (unsigned long long)c;
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) t += __shfl_xor(t, x, 64);
  if ((threadIdx.x & 63) == 0 && t) atomicAdd(&job.ctl->total, t);   // integer sum: order-independent
}

template <int KCAP, int NTH>
__global__ __launch_bounds__(NTH) void knn_search_kernel(KnnJob job) {
  // the lane's best entries so far in the contract's order, `have` of them: one LDS column per lane (consecutive lanes, consecutive words:
  // conflict-free), indexed at run time by the insertion
  __shared__ double s_d[KCAP][NTH];
  __shared__ int s_i[KCAP][NTH];
#define LD(t) s_d[t][threadIdx.x]
#define LI(t) s_i[t][threadIdx.x]
  const int i = blockIdx.x * NTH + threadIdx.x;
  long long row = 0;
  double qx = 0, qy = 0, qz = 0;
  const bool in_range = i < job.m;
  const bool active = lane_query(job, i, &row, &qx, &qy, &qz);
  int have = 0;
  if (in_range && job.q && !active) row = job.order ? job.order[i] : i;
  if (active && job.g.n > 0) {
    const int L = job.k;           // <= KCAP
    double wd = INFINITY; int wi = 0x7fffffff;   // the list's last entry once it is full; until then (+inf, max): everything enters
    const bool rad = job.rad_on != 0;
    const double B2 = job.B2;
    auto offer = [&](double d, const PointRec* p) {
      const int j = (int)p->idx;
      if (rad && !(d < B2)) return;
      if (!(d < wd || (d == wd && j <= wi))) return;   // (wd, wi): nothing after it in the order is among the first k
      int pos = have < L ? have : L - 1;
      while (pos > 0) {
        const double e = LD(pos - 1); const int ei = LI(pos - 1);
        if (!(e > d || (e == d && ei > j))) break;
        LD(pos) = e; LI(pos) = ei;
        --pos;
      }
      LD(pos) = d; LI(pos) = j;
      if (have < L) ++have;
      if (have == L) { wd = LD(L - 1); wi = LI(L - 1); }
    };
    // everything is offered again: the list empties, but (wd, wi) stays -- if the list was full its last entry is a real point, so the k-th
    // candidate is not after it, and that entry itself enters again (j <= wi)
    auto reset = [&]() { have = 0; };
    // a box whose lower bound exceeds wd holds only points after (wd, wi); one at or beyond B2 holds no candidate
    auto open = [&](double lb) { return !(lb > wd) && !(rad && !(lb < B2)); };
    // exact iff the k-th entry is strictly inside the scanned block (every point not offered is >= m away, so it can neither beat nor TIE
    // an entry); with a radius also once everything within the radius has been offered, full list or not
    auto stop = [&](double m2) { return (have == L && wd < m2) || (rad && B2 <= m2); };
    // at least k points are at most ub away: nothing beyond (ub, any index) is among the first k candidates (with a radius: if ub < B2
    // those k points are candidates themselves, otherwise everything beyond ub is outside the radius anyway)
    auto seed = [&](double ub) { if (ub < wd) { wd = ub; wi = 0x7fffffff; } };
    traverse(job.g, job.tree, qx, qy, qz, L, offer, reset, stop, open, seed);
    if (have > 0 && LD(have - 1) == INFINITY) atomicOr(&job.ctl->flags, kFlagOverflow);
  }
  if (in_range) {
    const RowsView o = *job.rows;
    const size_t base = (size_t)row * (size_t)job.k;
    for (int t = 0; t < have; ++t) { o.idx[base + t] = LI(t); o.d2[base + t] = LD(t); }
    for (int t = have; t < job.k; ++t) { o.idx[base + t] = -1; o.d2[base + t] = INFINITY; }
    o.cnt[row] = have;
  }
#undef LD
#undef LI
  add_total(job, have);
}

// all mode: FILL = false counts the candidates of every row, FILL = true stores them (same traversal, same visiting order)
template <bool FILL>
__global__ __launch_bounds__(128) void knn_all_kernel(KnnJob job) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  long long row = 0;
  double qx = 0, qy = 0, qz = 0;
  const bool in_range = i < job.m;
  const bool active = lane_query(job, i, &row, &qx, &qy, &qz);
  if (in_range && job.q && !active) row = job.order ? job.order[i] : i;
  int c = 0;
  if (active && job.g.n > 0) {
    const double B2 = job.B2;
    long long base = 0; int cap = 0;
    if (FILL) { base = job.off[row]; cap = (int)(job.off[row + 1] - base); }
    auto offer = [&](double d, const PointRec* p) {
      if (!(d < B2)) return;
      if (FILL) {
        if (c < cap) { job.eidx[base + c] = (int)p->idx; job.ed2[base + c] = d; }   // (c < cap always: the count pass offered the same points)
      }
      ++c;
    };
    auto reset = [&]() { c = 0; };
    auto stop = [&](double m2) { return B2 <= m2; };
    auto open = [&](double lb) { return lb < B2; };
    auto seed = [&](double) {};
    traverse(job.g, job.tree, qx, qy, qz, 0, offer, reset, stop, open, seed);
  }
  if (!FILL && in_range) { job.cnt[row] = c; job.cnt64[row] = c; }
  if (!FILL) add_total(job, c);
}

// all mode: one wave per row; entry e goes to its rank under (d2, index).  The pairs of a row are distinct (distinct indices), so the ranks
// are a permutation of 0 .. len-1 whatever the visiting order was.
__global__ __launch_bounds__(VT) void knn_order_kernel(const long long* __restrict__ off, int m, const int* __restrict__ eidx, const double* __restrict__ ed2,
                                                       int* __restrict__ idx, double* __restrict__ d2) {
  const int row = blockIdx.x * (VT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;
  const long long base = off[row];
  const int len = (int)(off[row + 1] - base);
  for (int e = lane; e < len; e += 64) {
    const double d = ed2[base + e]; const int j = eidx[base + e];
    int rank = 0;
    for (int f = 0; f < len; ++f) {
      const double df = ed2[base + f]; const int jf = eidx[base + f];
      rank += (df < d || (df == d && jf < j)) ? 1 : 0;
    }
    idx[base + rank] = j; d2[base + rank] = d;
  }
}

// query mode: the linear index of the clamped home cell (x fastest) and the query's id; a non-finite query gets key 0 (the search flags it)
__global__ __launch_bounds__(VT) void knn_key_kernel(const double* __restrict__ q, int m, GridView g, unsigned long long* __restrict__ key, int* __restrict__ ord) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= m) return;
  const double x = q[3 * (size_t)i], y = q[3 * (size_t)i + 1], z = q[3 * (size_t)i + 2];
  unsigned long long k = 0;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    const unsigned long long cx = home_cell(x, g.ox, g.inv_h, g.dx), cy = home_cell(y, g.oy, g.inv_h, g.dy), cz = home_cell(z, g.oz, g.inv_h, g.dz);
    k = (cz * (unsigned long long)g.dy + cy) * (unsigned long long)g.dx + cx;   // < 2^63: every dimension is < 2^21
  }
  key[i] = k; ord[i] = i;
}

// an empty frame: every row is padding; the queries are still checked
__global__ __launch_bounds__(VT) void knn_empty_kernel(const double* __restrict__ q, int m, int k, int* __restrict__ cnt, int* __restrict__ idx, double* __restrict__ d2,
                                                       long long* __restrict__ off, KnnCtl* __restrict__ ctl) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i >= m) return;
  if (q && !(isfinite(q[3 * (size_t)i]) && isfinite(q[3 * (size_t)i + 1]) && isfinite(q[3 * (size_t)i + 2]))) atomicOr(&ctl->flags, kFlagNonFinite);
  cnt[i] = 0;
  for (int t = 0; t < k; ++t) { idx[(size_t)i * k + t] = -1; d2[(size_t)i * k + t] = INFINITY; }
  if (k == 0) off[i] = 0;   // (all mode; off[m] is written by the host's memset)
}

__global__ __launch_bounds__(VT) void knn_rowoff_kernel(long long* __restrict__ off, int m, int k) {
  const int i = blockIdx.x * VT + threadIdx.x;
  if (i <= m) off[i] = (long long)i * k;
}

int launch_search(hipStream_t st, const KnnJob& j) {
  // one LDS column of 12 B entries per lane: 12 / 24 / 48 KiB per 128-lane workgroup at capacity 8 / 16 / 32, 48 KiB per 64-lane workgroup at 64
  if (j.k <= 8) hipLaunchKernelGGL((knn_search_kernel<8, 128>), dim3(grid_of(j.m, 128)), dim3(128), 0, st, j);
  else if (j.k <= 16) hipLaunchKernelGGL((knn_search_kernel<16, 128>), dim3(grid_of(j.m, 128)), dim3(128), 0, st, j);
  else if (j.k <= 32) hipLaunchKernelGGL((knn_search_kernel<32, 128>), dim3(grid_of(j.m, 128)), dim3(128), 0, st, j);
  else hipLaunchKernelGGL((knn_search_kernel<64, 64>), dim3(grid_of(j.m, 64)), dim3(64), 0, st, j);
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

}  // namespace

long long knn_search(mvicp_ctx* c, const FrameDev& f, const double* queries, int queries_on_device, long long m_in, int k, double radius, double B2) {
  c->knn.m = -1;   // (the last result ends here; a failed call leaves none behind)
  const bool self = queries == nullptr, rad_on = radius > 0.0, all = k == 0;
  const int n = f.n;
  const int m = self ? n : (int)m_in;
  if (n > 0 && !f.has_grid) { set_error("the neighbour search needs the per-cloud hash structure%s%s", f.build_error.empty() ? "" : ": ", f.build_error.c_str()); return MVICP_ERR_STATE; }
  hipStream_t st = c->stream;
  const size_t M = (size_t)m;

  // the result: [control | cnt | off] in one buffer, the entries [idx | d2] in another (all mode sizes them after the count)
  const size_t off_cnt = 256, off_off = off_cnt + align256(4 * M), head_bytes = off_off + align256(8 * (M + 1));
  MV_CHECK(c->knn.dev.reserve(head_bytes));
  MV_CHECK(c->knn.pin.reserve(256));
  KnnCtl* d_ctl = reinterpret_cast<KnnCtl*>(c->knn.dev.p);
  KnnCtl* h_ctl = reinterpret_cast<KnnCtl*>(c->knn.pin.p);
  c->knn.cnt = reinterpret_cast<int*>(c->knn.dev.p + off_cnt);
  c->knn.off = reinterpret_cast<long long*>(c->knn.dev.p + off_off);
  MV_HIP(hipMemsetAsync(d_ctl, 0, sizeof(KnnCtl), st));
  if (m == 0) {
    MV_HIP(hipMemsetAsync(c->knn.off, 0, 8, st));
    MV_HIP(hipStreamSynchronize(st));
    c->knn.idx = nullptr; c->knn.d2 = nullptr;
    c->knn.m = 0; c->knn.k = k; c->knn.total = 0;
    return 0;
  }

  // scratch: [queries (host queries only) | key a | key b | order a | order b | cnt64 | rocprim storage]
  const bool order_on = !self && c->knn_order && n > 0;
  const size_t s_q = 0, s_ka = s_q + ((!self && !queries_on_device) ? align256(24 * M) : 0), s_kb = s_ka + (order_on ? align256(8 * M) : 0);
  const size_t s_oa = s_kb + (order_on ? align256(8 * M) : 0), s_ob = s_oa + (order_on ? align256(4 * M) : 0);
  const size_t s_c64 = s_ob + (order_on ? align256(4 * M) : 0), s_rp = s_c64 + (all ? align256(8 * (M + 1)) : 0);
  size_t sort_bytes = 0, scan_bytes = 0;
  int bits = 1;
  if (order_on) {
    const unsigned __int128 cells = (unsigned __int128)f.grid.dims[0] * (unsigned __int128)f.grid.dims[1] * (unsigned __int128)f.grid.dims[2];
    while (bits < 64 && ((unsigned __int128)1 << bits) < cells) ++bits;   // keys are < cells <= 2^bits
    MV_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr, M, 0, bits, st));
  }
  if (all) MV_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (long long*)nullptr, (long long*)nullptr, 0ll, M + 1, rocprim::plus<long long>(), st));
  MV_CHECK(c->knn.tmp.reserve(s_rp + std::max<size_t>(std::max(sort_bytes, scan_bytes), 256)));
  char* T = c->knn.tmp.p;
  const double* d_q = nullptr;
  if (!self) {
    if (queries_on_device) d_q = queries;
    else {
      MV_HIP(hipMemcpyAsync(T + s_q, queries, 24 * M, hipMemcpyHostToDevice, st));
      d_q = reinterpret_cast<const double*>(T + s_q);
    }
  }

  KnnJob j;
  std::memset(&j, 0, sizeof(j));
  const GridDev& g = f.grid;
  if (n > 0) {
    fill_grid_view(&j.g, g, n);
    MV_CHECK(stage_tree_view(g, c->knn.pin.p + kTreeOffset, c->knn.dev.p + kTreeOffset, st, &j.tree));
  }
  j.q = d_q; j.m = m; j.k = k; j.rad_on = rad_on ? 1 : 0; j.B2 = B2;
  j.cnt = c->knn.cnt; j.ctl = d_ctl;
  if (order_on) {
    ProfScope ps(c, "knn_key", 44.0 * m);
    unsigned long long* key_a = reinterpret_cast<unsigned long long*>(T + s_ka); unsigned long long* key_b = reinterpret_cast<unsigned long long*>(T + s_kb);
    int* ord_a = reinterpret_cast<int*>(T + s_oa); int* ord_b = reinterpret_cast<int*>(T + s_ob);
    hipLaunchKernelGGL(knn_key_kernel, dim3(grid_of(m, VT)), dim3(VT), 0, st, d_q, m, j.g, key_a, ord_a);
    MV_HIP(hipGetLastError());
    size_t tb = sort_bytes;
    MV_HIP(rocprim::radix_sort_pairs(T + s_rp, tb, key_a, key_b, ord_a, ord_b, M, 0, bits, st));
    j.order = ord_b;
  }

  auto check_flags = [&](unsigned int flags) {
    if (flags & kFlagNonFinite) { set_error("knn search: a query coordinate is not finite"); return MVICP_ERR_ARG; }
    if (flags & kFlagOverflow) { set_error("knn search: a neighbour distance is not finite (coordinates too large)"); return MVICP_ERR_ARG; }
    return MVICP_OK;
  };

  long long total = 0;
  if (!all) {
    const size_t E = M * (size_t)k, off_d2 = align256(4 * E);
    MV_CHECK(c->knn.ent.reserve(off_d2 + align256(8 * E)));
    c->knn.idx = reinterpret_cast<int*>(c->knn.ent.p); c->knn.d2 = reinterpret_cast<double*>(c->knn.ent.p + off_d2);
    RowsView* h_rows = reinterpret_cast<RowsView*>(c->knn.pin.p + kRowsOffset);
    h_rows->cnt = c->knn.cnt; h_rows->idx = c->knn.idx; h_rows->d2 = c->knn.d2;
    MV_HIP(hipMemcpyAsync(c->knn.dev.p + kRowsOffset, h_rows, sizeof(RowsView), hipMemcpyHostToDevice, st));
    j.rows = reinterpret_cast<const RowsView*>(c->knn.dev.p + kRowsOffset);
    {
      ProfScope ps(c, "knn_search", (36.0 + 12.0 * k) * m);
      if (n > 0) MV_CHECK(launch_search(st, j));
      else {
        hipLaunchKernelGGL(knn_empty_kernel, dim3(grid_of(m, VT)), dim3(VT), 0, st, d_q, m, k, c->knn.cnt, c->knn.idx, c->knn.d2, c->knn.off, d_ctl);
        MV_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(knn_rowoff_kernel, dim3(grid_of((long long)m + 1, VT)), dim3(VT), 0, st, c->knn.off, m, k);
      MV_HIP(hipGetLastError());
    }
    MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(KnnCtl), hipMemcpyDeviceToHost, st));
    MV_HIP(hipStreamSynchronize(st));
    MV_CHECK(check_flags(h_ctl->flags));
    total = (long long)h_ctl->total;
  } else {
    long long* cnt64 = reinterpret_cast<long long*>(T + s_c64);
    j.cnt64 = cnt64;
    if (n > 0) {
      ProfScope ps(c, "knn_count", 36.0 * m);
      MV_HIP(hipMemsetAsync(cnt64 + M, 0, 8, st));
      hipLaunchKernelGGL(knn_all_kernel<false>, dim3(grid_of(m, 128)), dim3(128), 0, st, j);
      MV_HIP(hipGetLastError());
      size_t tb = scan_bytes;
      MV_HIP(rocprim::exclusive_scan(T + s_rp, tb, cnt64, c->knn.off, 0ll, M + 1, rocprim::plus<long long>(), st));
    } else {
      MV_HIP(hipMemsetAsync(c->knn.off + M, 0, 8, st));
      hipLaunchKernelGGL(knn_empty_kernel, dim3(grid_of(m, VT)), dim3(VT), 0, st, d_q, m, 0, j.cnt, (int*)nullptr, (double*)nullptr, c->knn.off, d_ctl);
      MV_HIP(hipGetLastError());
    }
    MV_HIP(hipMemcpyAsync(h_ctl, d_ctl, sizeof(KnnCtl), hipMemcpyDeviceToHost, st));
    MV_HIP(hipStreamSynchronize(st));
    MV_CHECK(check_flags(h_ctl->flags));
    total = (long long)h_ctl->total;
    if (total >= (1ll << 31)) { set_error("knn search: %lld neighbours in all: all mode returns fewer than 2^31 (smaller radius?)", total); return MVICP_ERR_ARG; }
    c->knn.idx = nullptr; c->knn.d2 = nullptr;
    if (total > 0) {
      // entries: [idx | d2] sorted, behind them [idx | d2] in visiting order
      const size_t E = (size_t)total, o_d2 = align256(4 * E), o_ti = o_d2 + align256(8 * E), o_td = o_ti + align256(4 * E);
      MV_CHECK(c->knn.ent.reserve(o_td + align256(8 * E)));
      c->knn.idx = reinterpret_cast<int*>(c->knn.ent.p); c->knn.d2 = reinterpret_cast<double*>(c->knn.ent.p + o_d2);
      j.off = c->knn.off; j.eidx = reinterpret_cast<int*>(c->knn.ent.p + o_ti); j.ed2 = reinterpret_cast<double*>(c->knn.ent.p + o_td);
      {
        ProfScope ps(c, "knn_fill", 36.0 * m + 12.0 * total);
        hipLaunchKernelGGL(knn_all_kernel<true>, dim3(grid_of(m, 128)), dim3(128), 0, st, j);
      }
      MV_HIP(hipGetLastError());
      {
        ProfScope ps(c, "knn_order", 24.0 * total);
        hipLaunchKernelGGL(knn_order_kernel, dim3(grid_of(m, VT / 64)), dim3(VT), 0, st, c->knn.off, m, j.eidx, j.ed2, c->knn.idx, c->knn.d2);
      }
      MV_HIP(hipGetLastError());
      MV_HIP(hipStreamSynchronize(st));
    }
  }
  c->knn.m = m; c->knn.k = k; c->knn.total = total;
  return total;
}

}  // namespace mvicp
