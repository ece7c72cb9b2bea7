// Batched coarse poses (mvicp_coarse_pairs): for every edge (a, b) of a list over n_sets descriptor / point sets the chain
//   mvicp_feature_match(desc_a, desc_b) -> mvicp_match_pairs -> P = xyz_a[pairs[:,0]], Q = xyz_b[pairs[:,1]] -> mvicp_consensus(P, Q, seeds[e])
// in one call, byte for byte what the chain of single calls gives.  The contract is that reduction (include/mvicp.h); the arithmetic is the
// device functions of match_tile.h and cons_pose.h, shared with match.hip and consensus.hip.  DESIGN.md §3.12.
//
//   1  coarse_match<33> / coarse_match_generic   one launch over a flat work table of (table, left-row block, chunk) records.  A table is
//                         an ordered set pair (L, R): the best two rows of R for every row of L.  Each distinct table is computed once:
//                         the forward table of edge (i, j) is the backward table of edge (j, i).  No workgroup is launched for padding.
//   2  coarse_merge       one launch over (table, left-row block) records: the best two over the chunks of each row
//   3  coarse_rule        one workgroup per edge: the pair rule per row of the source set, an order-preserving compaction (ballot + a
//                         scan over the four waves + a running base), pairs / P / Q written to the edge's segment, c_e to device memory
//   4  coarse_hyp         grid (H / 256, E), c_e read from device memory; fewer than three pairs reject every hypothesis at the index
//                         check, which precedes every load
//   5  coarse_score       one launch over (edge, slot block, pair chunk) records built from the (c_e, accepted_e) the host has fetched:
//                         the one wait of the call that is not its end
//   6  coarse_pick / coarse_flags   the edge on blockIdx.y; the result records
#include <map>
#include <utility>
#include <vector>

#include "common.h"
#include "cons_pose.h"
#include "match_tile.h"

namespace mvicp {

namespace {

using match_tile::Best2;
constexpr int kThreads = 256;
constexpr int kPairTile = 256;     // pairs per LDS tile of the scoring pass
constexpr int kWantBlocks = 2048;  // the scoring pass splits the pairs until the call has about this many workgroups
constexpr int kMaxChunks = 65535;

struct MatchWork { unsigned long long part; int l_off, m, r_off, lo, hi, row0, y, pad; };   // part: Best2 index of the table's first partial list
struct MergeWork { unsigned long long part, out; int m, chunks, row0, pad; };               // out: row index of the table's first result row
struct EdgeRec { unsigned long long fwd, bwd, seg, seed; int a_off, m, b_off, n; };        // fwd / bwd: first result rows of the two tables
struct ScoreWork { int edge, slot0, lo, hi; };
struct EdgeCtl { int c, n_acc; unsigned long long key; };
static_assert(sizeof(MatchWork) == 40 && sizeof(MergeWork) == 32 && sizeof(EdgeRec) == 48 && sizeof(ScoreWork) == 16 && sizeof(EdgeCtl) == 16, "record sizes");
static_assert(sizeof(mvicp_coarse_edge) == 144, "mvicp_coarse_edge is 144 bytes");

template <int DIM>
__global__ __launch_bounds__(match_tile::kThreads) void coarse_match(const MatchWork* __restrict__ work, const double* __restrict__ desc,
                                                                     Best2* __restrict__ part) {
  __shared__ double Bs[match_tile::kTile * match_tile::RegTile<DIM>::LD];
  const MatchWork w = work[blockIdx.x];
  const long long i = (long long)w.row0 + threadIdx.x;
  const bool live = i < w.m;
  double d0 = INFINITY, d1 = INFINITY; int j0 = -1, j1 = -1;
  match_tile::scan_reg<DIM>(desc + (size_t)w.l_off * DIM, i, live, desc + (size_t)w.r_off * DIM, w.lo, w.hi, Bs, d0, j0, d1, j1);
  if (live) { Best2* o = part + (w.part + (size_t)w.y * w.m + i); o->d0 = d0; o->d1 = d1; o->j0 = j0; o->j1 = j1; }
}

__global__ __launch_bounds__(match_tile::kGenRows) void coarse_match_generic(const MatchWork* __restrict__ work, const double* __restrict__ desc, int dim,
                                                                             Best2* __restrict__ part) {
  __shared__ double As[match_tile::kMaxDim * match_tile::kGenRows];   // [c][row]
  __shared__ double Bs[match_tile::kGenTile * match_tile::kMaxDim];   // [row][c]
  const MatchWork w = work[blockIdx.x];
  const long long i = (long long)w.row0 + threadIdx.x;
  const bool live = i < w.m;
  double d0 = INFINITY, d1 = INFINITY; int j0 = -1, j1 = -1;
  match_tile::scan_generic(desc + (size_t)w.l_off * dim, w.m, w.row0, desc + (size_t)w.r_off * dim, w.lo, w.hi, dim, As, Bs, d0, j0, d1, j1);
  if (live) { Best2* o = part + (w.part + (size_t)w.y * w.m + i); o->d0 = d0; o->d1 = d1; o->j0 = j0; o->j1 = j1; }
}

__global__ __launch_bounds__(kThreads) void coarse_merge(const MergeWork* __restrict__ work, const Best2* __restrict__ part, int* __restrict__ idx,
                                                         double* __restrict__ d2) {
  const MergeWork w = work[blockIdx.x];
  const long long i = (long long)w.row0 + threadIdx.x;
  if (i >= w.m) return;
  double d0 = INFINITY, d1 = INFINITY; int j0 = -1, j1 = -1;
  match_tile::merge_row(part + w.part, (size_t)w.m, (size_t)i, w.chunks, d0, j0, d1, j1);
  const size_t o = 2 * (w.out + (size_t)i);
  idx[o] = j0; idx[o + 1] = j1;
  d2[o] = d0; d2[o + 1] = d1;
}

// the pair rule of mvicp_match_pairs for every row of the edge's source set, compacted in ascending i
__global__ __launch_bounds__(kThreads) void coarse_rule(const EdgeRec* __restrict__ edges, const int* __restrict__ idx, const double* __restrict__ d2,
                                                        const double* __restrict__ xyz, int mutual, int use_ratio, double r2, int* __restrict__ pairs,
                                                        double* __restrict__ P, double* __restrict__ Q, EdgeCtl* __restrict__ ctl) {
  __shared__ int wave_sum[kThreads / 64];
  const EdgeRec e = edges[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int base = 0;   // pairs kept in the rows before this block of rows (the same value in every thread)
  for (int row0 = 0; row0 < e.m; row0 += kThreads) {
    const int i = row0 + (int)threadIdx.x;
    bool keep = false; int j = -1;
    if (i < e.m) {
      j = idx[2 * (e.fwd + (size_t)i)];
      keep = j >= 0;
      if (keep && mutual) keep = idx[2 * (e.bwd + (size_t)j)] == i;
      if (keep && use_ratio) keep = d2[2 * (e.fwd + (size_t)i)] <= __dmul_rn(r2, d2[2 * (e.fwd + (size_t)i) + 1]);
    }
    const unsigned long long mask = __ballot(keep);
    __syncthreads();   // (the sums of the last block of rows have been read)
    if (lane == 0) wave_sum[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) { const int s = wave_sum[w]; before += w < wave ? s : 0; all += s; }
    if (keep) {
      const size_t k = e.seg + (size_t)(base + before + __popcll(mask & ((1ull << lane) - 1ull)));
      pairs[2 * k] = i; pairs[2 * k + 1] = j;
      const double* p = xyz + 3 * ((size_t)e.a_off + (size_t)i);
      const double* q = xyz + 3 * ((size_t)e.b_off + (size_t)j);
      P[3 * k] = p[0]; P[3 * k + 1] = p[1]; P[3 * k + 2] = p[2];
      Q[3 * k] = q[0]; Q[3 * k + 1] = q[1]; Q[3 * k + 2] = q[2];
    }
    base += all;
  }
  if (threadIdx.x == 0) { ctl[blockIdx.x].c = base; ctl[blockIdx.x].n_acc = 0; ctl[blockIdx.x].key = 0ull; }
}

__global__ __launch_bounds__(kThreads) void coarse_hyp(const EdgeRec* __restrict__ edges, const double* __restrict__ P, const double* __restrict__ Q, int H,
                                                       double s2, int* __restrict__ count, int* __restrict__ hidx, EdgeCtl* __restrict__ ctl) {
  const int e = blockIdx.y;
  const int h = (int)(blockIdx.x * kThreads + threadIdx.x), lane = threadIdx.x & 63;   // (H <= 2^24)
  const EdgeRec er = edges[e];
  const int c = ctl[e].c;
  // c < 3: two of the three indices are equal and the hypothesis is rejected before any load from the (possibly empty) segment
  const bool ok = h < H && cons_pose::hypothesis<false>(P + 3 * er.seg, Q + 3 * er.seg, (unsigned long long)c, er.seed, (unsigned int)h, s2, nullptr, nullptr);
  if (h < H) count[(size_t)e * H + h] = ok ? 0 : -1;
  const unsigned long long mask = __ballot(ok);
  if (mask == 0ull) return;
  const int first = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == first) base = atomicAdd(&ctl[e].n_acc, __popcll(mask));
  base = __shfl(base, first);
  if (ok) hidx[(size_t)e * H + base + __popcll(mask & ((1ull << lane) - 1ull))] = h;
}

__global__ __launch_bounds__(kThreads) void coarse_score(const ScoreWork* __restrict__ work, const EdgeRec* __restrict__ edges, const double* __restrict__ P,
                                                         const double* __restrict__ Q, int H, double s2, double tau2, const int* __restrict__ hidx,
                                                         const EdgeCtl* __restrict__ ctl, int* __restrict__ count) {
  __shared__ double Sp[3 * kPairTile];
  __shared__ double Sq[3 * kPairTile];
  const ScoreWork w = work[blockIdx.x];
  const EdgeRec er = edges[w.edge];
  const int c = ctl[w.edge].c, n_acc = ctl[w.edge].n_acc;
  const double* Pe = P + 3 * er.seg;
  const double* Qe = Q + 3 * er.seg;
  const int slot = w.slot0 + (int)threadIdx.x;
  bool live = slot < n_acc;
  const int h = live ? hidx[(size_t)w.edge * H + slot] : 0;
  double R[9], t[3];
  if (live) live = cons_pose::hypothesis<true>(Pe, Qe, (unsigned long long)c, er.seed, (unsigned int)h, s2, R, t);   // (always accepted: coarse_hyp decided with the same code)
  if (!live) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
  }
  const int hi = w.hi < c ? w.hi : c;
  int cnt = 0;
  for (int base = w.lo; base < hi; base += kPairTile) {
    const int rows = hi - base < kPairTile ? hi - base : kPairTile;
    __syncthreads();   // (the last tile has been read by every wave)
    for (int e = threadIdx.x; e < 3 * rows; e += kThreads) { Sp[e] = Pe[3 * (size_t)base + e]; Sq[e] = Qe[3 * (size_t)base + e]; }
    __syncthreads();
    for (int r = 0; r < rows; ++r) cnt += cons_pose::inlier(R, t, Sp + 3 * r, Sq + 3 * r, tau2) ? 1 : 0;
  }
  if (live && cnt) atomicAdd(&count[(size_t)w.edge * H + h], cnt);
}

// max over the keys (count + 1) << 32 | (2^32 - 1 - h): the largest count, the lowest h
__global__ __launch_bounds__(kThreads) void coarse_pick(const int* __restrict__ count, int H, EdgeCtl* __restrict__ ctl) {
  const int e = blockIdx.y;
  const int h = (int)(blockIdx.x * kThreads + threadIdx.x);
  const int n = h < H ? count[(size_t)e * H + h] : -1;
  unsigned long long key = n >= 0 ? ((unsigned long long)((unsigned int)n + 1u) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)h) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&ctl[e].key, key);
}

// the winner's pose once more, its inlier flags, the result record; blocks past an edge's pairs only leave (block 0 writes the record)
__global__ __launch_bounds__(kThreads) void coarse_flags(const EdgeRec* __restrict__ edges, const double* __restrict__ P, const double* __restrict__ Q, double s2,
                                                         double tau2, const EdgeCtl* __restrict__ ctl, unsigned char* __restrict__ flags,
                                                         mvicp_coarse_edge* __restrict__ res) {
  const int e = blockIdx.y;
  const int c = ctl[e].c;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= c && i != 0) return;
  const EdgeRec er = edges[e];
  const double* Pe = P + 3 * er.seg;
  const double* Qe = Q + 3 * er.seg;
  const unsigned long long key = ctl[e].key;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  int best = -1, n = 0;
  if (key) {
    best = (int)(0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull));
    n = (int)(key >> 32) - 1;
    (void)cons_pose::hypothesis<true>(Pe, Qe, (unsigned long long)c, er.seed, (unsigned int)best, s2, R, t);
  }
  if (i < c) flags[er.seg + (size_t)i] = key && cons_pose::inlier(R, t, Pe + 3 * i, Qe + 3 * i, tau2) ? 1 : 0;
  if (i == 0) {
    mvicp_coarse_edge* o = res + e;
    o->pairs = c; o->best = best; o->count = n; o->accepted = ctl[e].n_acc;
#pragma unroll
    for (int col = 0; col < 3; ++col) {   // column-major 4 x 4
#pragma unroll
      for (int r = 0; r < 3; ++r) o->pose[4 * col + r] = R[3 * r + col];
      o->pose[4 * col + 3] = 0.0;
    }
    o->pose[12] = t[0]; o->pose[13] = t[1]; o->pose[14] = t[2]; o->pose[15] = 1.0;
  }
}

__global__ __launch_bounds__(kThreads) void coarse_finite(const double* __restrict__ v, size_t count, int* __restrict__ flag) {
  bool bad = false;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < count; e += (size_t)gridDim.x * kThreads) bad |= !isfinite(v[e]);
  if (bad) atomicOr(flag, 1);
}

// rows of the right operand per chunk and the number of chunks for `right` > 0 rows: the rule of match.hip
void chunking(const mvicp_ctx* c, long long right, int* chunk, int* chunks) {
  long long ch = c->match_chunk > 0 ? c->match_chunk : 1;
  if ((right + ch - 1) / ch > kMaxChunks) ch = (right + kMaxChunks - 1) / kMaxChunks;
  if (ch > right) ch = right > 0 ? right : 1;
  *chunk = (int)ch;
  *chunks = (int)((right + ch - 1) / ch);
}

struct Table { int L, R, chunk, chunks; size_t part, out; };

}  // namespace

long long coarse_pairs(mvicp_ctx* c, const double* desc, int desc_on_device, const double* xyz, int xyz_on_device, const long long* offsets, int n_sets, int dim,
                       int n_edges, const int* src, const int* dst, const unsigned long long* seeds, int mutual, double ratio, long long H, double tau,
                       double edge_sim, mvicp_coarse_edge* results) {
  c->coarse.edges = -1;   // (the last result ends here; a failed call leaves none behind)
  hipStream_t st = c->stream;
  const size_t E = (size_t)n_edges, NH = (size_t)H, total = (size_t)offsets[n_sets];
  auto rows_of = [&](int s) { return (int)(offsets[s + 1] - offsets[s]); };

  // the distinct tables: (L, R) = the best two rows of R for every row of L
  std::vector<Table> tables;
  std::map<std::pair<int, int>, size_t> table_of;
  auto table = [&](int L, int R) -> size_t {
    const auto it = table_of.find({L, R});
    if (it != table_of.end()) return it->second;
    table_of[{L, R}] = tables.size();
    tables.push_back(Table{L, R, 1, 0, 0, 0});
    return tables.size() - 1;
  };
  std::vector<size_t> e_fwd(E), e_bwd(E);
  for (size_t e = 0; e < E; ++e) { e_fwd[e] = table(src[e], dst[e]); e_bwd[e] = mutual ? table(dst[e], src[e]) : e_fwd[e]; }
  const bool reg = dim == 33;
  const int lrows = reg ? match_tile::kThreads : match_tile::kGenRows;
  size_t n_part = 0, n_out = 0;
  std::vector<MatchWork> mwork;
  std::vector<MergeWork> gwork;
  double match_bytes = 0.0, merge_bytes = 0.0;
  for (Table& t : tables) {
    const int m = rows_of(t.L), n = rows_of(t.R);
    t.part = n_part; t.out = n_out;
    if (m > 0 && n > 0) chunking(c, n, &t.chunk, &t.chunks);
    n_part += (size_t)m * t.chunks; n_out += (size_t)m;
    for (int row0 = 0; row0 < m; row0 += lrows)
      for (int y = 0; y < t.chunks; ++y) {
        const long long lo = (long long)y * t.chunk, hi = lo + t.chunk < (long long)n ? lo + t.chunk : (long long)n;
        mwork.push_back(MatchWork{(unsigned long long)t.part, (int)offsets[t.L], m, (int)offsets[t.R], (int)lo, (int)hi, row0, y, 0});
      }
    for (int row0 = 0; row0 < m; row0 += kThreads) gwork.push_back(MergeWork{(unsigned long long)t.part, (unsigned long long)t.out, m, t.chunks, row0, 0});
    const double wgs = (m + lrows - 1) / lrows;
    match_bytes += 8.0 * dim * ((double)m * t.chunks + wgs * n) + sizeof(Best2) * (double)m * t.chunks;
    merge_bytes += (sizeof(Best2) * (double)t.chunks + 24.0) * m;
  }
  if (mwork.size() > 0x7FFFFFFFull || gwork.size() > 0x7FFFFFFFull) { set_error("coarse pairs: too many work records"); return MVICP_ERR_ARG; }

  // the edges and their segments (capacity: the rows of the source set)
  std::vector<EdgeRec> erec(E);
  std::vector<long long> seg(E + 1, 0);
  for (size_t e = 0; e < E; ++e) {
    const int a = src[e], b = dst[e];
    erec[e] = EdgeRec{(unsigned long long)tables[e_fwd[e]].out, (unsigned long long)tables[e_bwd[e]].out, (unsigned long long)seg[e], seeds[e],
                      (int)offsets[a], rows_of(a), (int)offsets[b], rows_of(b)};
    seg[e + 1] = seg[e] + rows_of(a);
  }
  const size_t S = (size_t)seg[E];

  // the result: [pairs S x 2 ints | flags S bytes]
  const size_t off_flags = align256(8 * S);
  MV_CHECK(c->coarse.dev.reserve(off_flags + align256(S) + 256));
  c->coarse.pairs = reinterpret_cast<int*>(c->coarse.dev.p);
  c->coarse.flags = reinterpret_cast<unsigned char*>(c->coarse.dev.p + off_flags);
  // scratch: [flag | desc staged | xyz staged | partial lists | table idx | table d2 | P | Q | count E x H | accepted E x H | ctl E | results E |
  //           edges | match work | merge work]
  size_t off = 256;
  auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
  const size_t o_desc = take(desc_on_device ? 0 : 8 * total * dim), o_xyz = take(xyz_on_device ? 0 : 24 * total);
  const size_t o_part = take(sizeof(Best2) * n_part), o_idx = take(8 * n_out), o_d2 = take(16 * n_out), o_P = take(24 * S), o_Q = take(24 * S);
  const size_t o_count = take(4 * E * NH), o_hidx = take(4 * E * NH), o_ctl = take(sizeof(EdgeCtl) * E), o_res = take(sizeof(mvicp_coarse_edge) * E);
  const size_t o_edges = take(sizeof(EdgeRec) * E), o_mwork = take(sizeof(MatchWork) * mwork.size()), o_gwork = take(sizeof(MergeWork) * gwork.size());
  MV_CHECK(c->coarse.tmp.reserve(off));
  char* T = c->coarse.tmp.p;
  int* flag = reinterpret_cast<int*>(T);
  const double* d_desc = desc; const double* d_xyz = xyz;
  if (!desc_on_device && total) { MV_HIP(hipMemcpyAsync(T + o_desc, desc, 8 * total * dim, hipMemcpyHostToDevice, st)); d_desc = reinterpret_cast<const double*>(T + o_desc); }
  if (!xyz_on_device && total) { MV_HIP(hipMemcpyAsync(T + o_xyz, xyz, 24 * total, hipMemcpyHostToDevice, st)); d_xyz = reinterpret_cast<const double*>(T + o_xyz); }
  MV_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  if (E) MV_HIP(hipMemcpyAsync(T + o_edges, erec.data(), sizeof(EdgeRec) * E, hipMemcpyHostToDevice, st));
  if (!mwork.empty()) MV_HIP(hipMemcpyAsync(T + o_mwork, mwork.data(), sizeof(MatchWork) * mwork.size(), hipMemcpyHostToDevice, st));
  if (!gwork.empty()) MV_HIP(hipMemcpyAsync(T + o_gwork, gwork.data(), sizeof(MergeWork) * gwork.size(), hipMemcpyHostToDevice, st));
  // the finite check runs with the rest and is read at the call's one intermediate wait: every kernel below is memory-safe on any input
  // (indices come from comparisons and the sampler, never from the values)
  const double* checked[2] = {d_desc, d_xyz};
  const size_t counts[2] = {total * dim, 3 * total};
  for (int t = 0; t < 2; ++t)
    if (counts[t]) {
      const size_t wgs = (counts[t] + kThreads - 1) / kThreads;
      hipLaunchKernelGGL(coarse_finite, dim3((unsigned int)(wgs < 4096 ? wgs : 4096)), dim3(kThreads), 0, st, checked[t], counts[t], flag);
      MV_HIP(hipGetLastError());
    }
  Best2* part = reinterpret_cast<Best2*>(T + o_part);
  int* t_idx = reinterpret_cast<int*>(T + o_idx);
  double* t_d2 = reinterpret_cast<double*>(T + o_d2);
  double* P = reinterpret_cast<double*>(T + o_P);
  double* Q = reinterpret_cast<double*>(T + o_Q);
  int* count = reinterpret_cast<int*>(T + o_count);
  int* hidx = reinterpret_cast<int*>(T + o_hidx);
  EdgeCtl* ctl = reinterpret_cast<EdgeCtl*>(T + o_ctl);
  mvicp_coarse_edge* d_res = reinterpret_cast<mvicp_coarse_edge*>(T + o_res);
  const EdgeRec* d_edges = reinterpret_cast<const EdgeRec*>(T + o_edges);
  const MatchWork* d_mwork = reinterpret_cast<const MatchWork*>(T + o_mwork);
  const MergeWork* d_gwork = reinterpret_cast<const MergeWork*>(T + o_gwork);
  if (E == 0) {
    int h_flag = 0;
    MV_HIP(hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    MV_HIP(hipStreamSynchronize(st));
    if (h_flag) { set_error("a descriptor value or a coordinate is not finite"); return MVICP_ERR_ARG; }
    c->coarse.seg.assign(1, 0); c->coarse.cnt.clear();
    c->coarse.edges = 0;
    return 0;
  }
  if (!mwork.empty()) {
    ProfScope ps(c, "coarse_match", match_bytes + sizeof(MatchWork) * (double)mwork.size());
    if (reg) hipLaunchKernelGGL(coarse_match<33>, dim3((unsigned int)mwork.size()), dim3(match_tile::kThreads), 0, st, d_mwork, d_desc, part);
    else hipLaunchKernelGGL(coarse_match_generic, dim3((unsigned int)mwork.size()), dim3(match_tile::kGenRows), 0, st, d_mwork, d_desc, dim, part);
    MV_HIP(hipGetLastError());
  }
  if (!gwork.empty()) {
    ProfScope ps(c, "coarse_merge", merge_bytes + sizeof(MergeWork) * (double)gwork.size());
    hipLaunchKernelGGL(coarse_merge, dim3((unsigned int)gwork.size()), dim3(kThreads), 0, st, d_gwork, part, t_idx, t_d2);
    MV_HIP(hipGetLastError());
  }
  const double s2 = edge_sim * edge_sim, tau2 = tau * tau, r2 = ratio * ratio;
  const int use_ratio = !(ratio >= 1.0);
  {
    ProfScope ps(c, "coarse_rule", (8.0 + (mutual ? 4.0 : 0.0) + (use_ratio ? 16.0 : 0.0) + 8.0 + 96.0) * (double)S + 64.0 * E);
    hipLaunchKernelGGL(coarse_rule, dim3((unsigned int)E), dim3(kThreads), 0, st, d_edges, t_idx, t_d2, d_xyz, mutual ? 1 : 0, use_ratio, r2, c->coarse.pairs, P, Q, ctl);
    MV_HIP(hipGetLastError());
  }
  const dim3 block(kThreads), grid_h((unsigned int)((NH + kThreads - 1) / kThreads), (unsigned int)E);
  {
    ProfScope ps(c, "coarse_hyp", (8.0 * NH + 144.0 * NH) * E);   // count and the accepted list; six points per hypothesis
    hipLaunchKernelGGL(coarse_hyp, grid_h, block, 0, st, d_edges, P, Q, (int)H, s2, count, hidx, ctl);
    MV_HIP(hipGetLastError());
  }
  // the one wait that is not the end of the call: (c_e, accepted_e) of every edge size the scoring launch
  std::vector<EdgeCtl> h_ctl(E);
  int h_flag = 0;
  MV_HIP(hipMemcpyAsync(h_ctl.data(), ctl, sizeof(EdgeCtl) * E, hipMemcpyDeviceToHost, st));
  MV_HIP(hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (h_flag) { set_error("a descriptor value or a coordinate is not finite"); return MVICP_ERR_ARG; }
  long long slot_blocks = 0; int max_c = 0;
  for (size_t e = 0; e < E; ++e) { slot_blocks += (h_ctl[e].n_acc + kThreads - 1) / kThreads; max_c = h_ctl[e].c > max_c ? h_ctl[e].c : max_c; }
  std::vector<ScoreWork> swork;
  double score_bytes = 0.0;
  if (slot_blocks > 0) {
    const long long want = (kWantBlocks + slot_blocks - 1) / slot_blocks;   // pair chunks per slot block, at most one per tile
    for (size_t e = 0; e < E; ++e) {
      const int n_acc = h_ctl[e].n_acc, ce = h_ctl[e].c;
      if (n_acc <= 0) continue;
      const long long tiles = ((long long)ce + kPairTile - 1) / kPairTile;
      const long long gy = want < tiles ? want : tiles;
      const long long per_y = ((tiles + gy - 1) / gy) * kPairTile;   // (whole tiles)
      for (int slot0 = 0; slot0 < n_acc; slot0 += kThreads)
        for (long long lo = 0; lo < ce; lo += per_y) swork.push_back(ScoreWork{(int)e, slot0, (int)lo, (int)(lo + per_y < ce ? lo + per_y : ce)});
      score_bytes += 48.0 * ce * ((n_acc + kThreads - 1) / kThreads) + 148.0 * n_acc;
    }
    if (swork.size() > 0x7FFFFFFFull) { set_error("coarse pairs: too many scoring records"); return MVICP_ERR_ARG; }
    MV_CHECK(c->coarse.work.reserve(sizeof(ScoreWork) * swork.size()));
    MV_HIP(hipMemcpyAsync(c->coarse.work.p, swork.data(), sizeof(ScoreWork) * swork.size(), hipMemcpyHostToDevice, st));
    ProfScope ps(c, "coarse_score", score_bytes + sizeof(ScoreWork) * (double)swork.size());
    hipLaunchKernelGGL(coarse_score, dim3((unsigned int)swork.size()), block, 0, st, reinterpret_cast<const ScoreWork*>(c->coarse.work.p), d_edges, P, Q, (int)H, s2, tau2,
                       hidx, ctl, count);
    MV_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "coarse_pick", 4.0 * NH * E + 49.0 * (double)S + sizeof(mvicp_coarse_edge) * (double)E);
    hipLaunchKernelGGL(coarse_pick, grid_h, block, 0, st, count, (int)H, ctl);
    const unsigned int gx = (unsigned int)(max_c > 0 ? (max_c + kThreads - 1) / kThreads : 1);
    hipLaunchKernelGGL(coarse_flags, dim3(gx, (unsigned int)E), block, 0, st, d_edges, P, Q, s2, tau2, ctl, c->coarse.flags, d_res);
    MV_HIP(hipGetLastError());
  }
  std::vector<mvicp_coarse_edge> h_res(E);
  MV_HIP(hipMemcpyAsync(h_res.data(), d_res, sizeof(mvicp_coarse_edge) * E, hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  c->coarse.seg = seg;
  c->coarse.cnt.resize(E);
  for (size_t e = 0; e < E; ++e) { results[e] = h_res[e]; c->coarse.cnt[e] = h_res[e].pairs; }
  c->coarse.edges = n_edges;
  return n_edges;
}

}  // namespace mvicp
