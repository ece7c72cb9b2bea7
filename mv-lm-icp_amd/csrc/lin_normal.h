// The pipeline of the two normal-carrying objectives (linearize_sym.hip: symmetric; linearize_gicp.hip: plane-to-plane), written once: everything around
// the per-correspondence arithmetic of their kernels, and their host launch.  Each unit keeps its __global__ kernel, which is one call of
// linearize_normal_body with its accumulate step, and its launch_* function, which is one call of launch_linearize_normal.
//
// Operands: n_q (arrays 3-5) and q (arrays 7-9) from the operand stream, non-temporal; p from arrays 0-2 or, for an identity list, from the shared
// sorted source cloud (as linearize_kernel); n_p from the source frame's sorted normals at first[pos] — the stream is NOT widened — which for an identity
// list is position pos itself, three 16-B loads per pair like p.  Both cloud-side loads are ordinary cacheable loads: the edges of a source frame share them.
// The gather index of the step AFTER the next is loaded one step early, so its latency is not on the path of the prefetch that depends on it.
// Mapping, chunk tables, partial slots: those of linearize_kernel (launch_linearize's tables; the XCD interleave comes with them).
#pragma once
#include "lin_common.h"

namespace mvicp {

namespace {

// One 256-thread workgroup per chunk of one edge, two adjacent correspondences per lane per step, the next step's operands in flight during the
// arithmetic: linearize_kernel's mapping.  Register slots: 0-2 p, 3-5 n_q, 6-8 q, 9-11 n_p.
// accumulate(acc, A, t, lo, inv_a2, p (3), n_q (3), q (3), n_p (3)) adds one correspondence to the 28 sums; lo[0..8] are the low parts of A, lo[9..11] of t.
// LO_SCALAR picks the route of those 12 low parts.  false: through LDS like the high parts (srel[1]).  true: straight from global memory at a block-uniform
// address, before the barrier, and so by scalar loads into SGPRs instead of 24 VGPRs; srel then has one row.
template <bool ROBUST, bool LO_SCALAR, class Accumulate>
__device__ __forceinline__ void linearize_normal_body(const int* __restrict__ chunk_edge, const int* __restrict__ chunk_start, int chunk,
                                                      const int* __restrict__ count, const long long* __restrict__ cap_off, long long total_cap,
                                                      const double* __restrict__ rel, const double* __restrict__ rel_lo, const double* __restrict__ a_scale,
                                                      const double* __restrict__ stream, double* __restrict__ partials,
                                                      const double* const* __restrict__ src_pts, const double* const* __restrict__ src_nor,
                                                      const int* __restrict__ first, const int* __restrict__ nsrc,
                                                      const int* __restrict__ chunk_first, Accumulate accumulate) {
  const int e = chunk_edge[blockIdx.x];
  const int start = chunk_start[blockIdx.x];
  const int c = chunk_first[e] + start / chunk;   // the partial's slot: the chunk's place in its edge's run, whatever the launch order
  const int cnt = count[e];
  if (start >= cnt) return;
  const int end = min(cnt, start + chunk);
  double lo[kEdgeRel];
  if constexpr (LO_SCALAR) {
#pragma unroll
    for (int i = 0; i < kEdgeRel; ++i) lo[i] = rel_lo[(size_t)e * kEdgeRel + i];
  }
  __shared__ double srel[LO_SCALAR ? 1 : 2][kEdgeRel];
  __shared__ double red[NACC / 2][NT + 1];
  if (threadIdx.x < kEdgeRel) srel[0][threadIdx.x] = rel[(size_t)e * kEdgeRel + threadIdx.x];
  if constexpr (!LO_SCALAR) {
    if (threadIdx.x >= 32 && threadIdx.x < 32 + kEdgeRel) srel[1][threadIdx.x - 32] = rel_lo[(size_t)e * kEdgeRel + threadIdx.x - 32];
  }
  __syncthreads();
  double A[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] = srel[0][i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = srel[0][9 + i];
  if constexpr (!LO_SCALAR) {
#pragma unroll
    for (int i = 0; i < kEdgeRel; ++i) lo[i] = srel[1][i];
  }
  double inv_a2 = 1.0;
  if (ROBUST) { const double a = a_scale[e]; inv_a2 = 1.0 / (a * a); }

  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;

  const size_t base = (size_t)cap_off[e];  // multiple of 64 -> 16-B aligned double2 loads, 8-B aligned index pairs
  const double* __restrict__ s0 = stream + base;
  const int* __restrict__ fi = first + base;
  const double* __restrict__ sn = src_nor[e];   // the source frame's normals in its sorted order (non-null: check_evaluable)
  // identity list (count == N_src): p AND n_p are the source cloud's own arrays at position pos
  const double* __restrict__ sp = (src_pts != nullptr && cnt == nsrc[e]) ? src_pts[e] : nullptr;
  constexpr int NS = 12;
  // register slot j < 9 -> stream array: p = arrays 0-2, n_q = arrays 3-5, q = arrays 7-9
  auto arr = [](int j) { return j < 6 ? j : j + 1; };
  typedef double d2v __attribute__((ext_vector_type(2)));
  typedef int i2v __attribute__((ext_vector_type(2)));
  auto aos_pair = [](const double* __restrict__ b, int at, double2& v0, double2& v1, double2& v2) {   // rows at, at + 1 of an n x 3 array (at even)
    const double2 a = *reinterpret_cast<const double2*>(b + 3 * (size_t)at);
    const double2 m = *reinterpret_cast<const double2*>(b + 3 * (size_t)at + 2);
    const double2 z = *reinterpret_cast<const double2*>(b + 3 * (size_t)at + 4);
    v0 = make_double2(a.x, m.y); v1 = make_double2(a.y, z.x); v2 = make_double2(m.x, z.y);
  };
  // sorted positions of the source points of the pair at `at` (unused for an identity list)
  auto load_idx = [&](int2& ix, int at) {
    if (sp != nullptr) return;
    if (at + 1 < end) { const i2v k = __builtin_nontemporal_load(reinterpret_cast<const i2v*>(fi + at)); ix = make_int2(k.x, k.y); }
    else if (at < end) { ix = make_int2(fi[at], 0); }
  };
  auto load = [&](double2 (&v)[NS], int at, const int2& ix) {
    if (at + 1 < end) {
      if (sp != nullptr) {
        aos_pair(sp, at, v[0], v[1], v[2]);
        aos_pair(sn, at, v[9], v[10], v[11]);
      } else {
        const double* __restrict__ na = sn + 3 * (size_t)ix.x;
        const double* __restrict__ nb = sn + 3 * (size_t)ix.y;
#pragma unroll
        for (int j = 0; j < 3; ++j) v[9 + j] = make_double2(na[j], nb[j]);
      }
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        if (j < 3 && sp != nullptr) continue;
        const d2v x = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(s0 + (size_t)arr(j) * total_cap + at));   // read once per evaluation
        v[j] = make_double2(x.x, x.y);
      }
    } else if (at < end) {
      const double* __restrict__ na = sn + 3 * (size_t)(sp != nullptr ? at : ix.x);
#pragma unroll
      for (int j = 0; j < 3; ++j) { v[9 + j].x = na[j]; v[9 + j].y = 0.0; }
#pragma unroll
      for (int j = 0; j < 9; ++j) { v[j].x = (j < 3 && sp != nullptr) ? sp[3 * (size_t)at + j] : s0[(size_t)arr(j) * total_cap + at]; v[j].y = 0.0; }
    }
  };
  int pos = start + 2 * threadIdx.x;
  double2 cur[NS], nxt[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) { cur[j] = make_double2(0.0, 0.0); nxt[j] = make_double2(0.0, 0.0); }
  int2 ix = make_int2(0, 0), ix_next = make_int2(0, 0);
  load_idx(ix, pos);
  load_idx(ix_next, pos + 2 * NT);
  load(cur, pos, ix);
  while (pos < end) {
    const int npos = pos + 2 * NT;
    ix = ix_next;
    load_idx(ix_next, npos + 2 * NT);
    load(nxt, npos, ix);
    accumulate(acc, A, t, lo, inv_a2, cur[0].x, cur[1].x, cur[2].x, cur[3].x, cur[4].x, cur[5].x, cur[6].x, cur[7].x, cur[8].x, cur[9].x, cur[10].x, cur[11].x);
    if (pos + 1 < end)
      accumulate(acc, A, t, lo, inv_a2, cur[0].y, cur[1].y, cur[2].y, cur[3].y, cur[4].y, cur[5].y, cur[6].y, cur[7].y, cur[8].y, cur[9].y, cur[10].y, cur[11].y);
#pragma unroll
    for (int j = 0; j < NS; ++j) cur[j] = nxt[j];
    pos = npos;
  }
  block_reduce_store(acc, red, partials, c, false);
}

// The host side of both families: launch_linearize's source table, the table of the source frames' sorted normals, the low parts of the relative transforms,
// the accumulation kernel under the profile scope `scope`, and the plane family's expansion.  `what` names the family in the error text;
// launch(robust, chunk, d_lo, d_src, d_nor) is the unit's hipLaunchKernelGGL of its own kernel (the kernels sit in the units' anonymous namespaces).
template <class Launch>
static int launch_linearize_normal(mvicp_ctx* c, int robust, const char* scope, const char* what, Launch launch) {
  if (c->E == 0) return MVICP_OK;
  const int chunk = c->lin_chunk;
  if (c->n_chunks > 0) {
    const double bytes = sym_pass_bytes(c);
    // per-edge sorted source clouds (launch_linearize's table) and their normals, cached by content
    const double* const* d_src = nullptr;
    MV_CHECK(source_table(c, &d_src));
    std::vector<const double*> nor((size_t)c->E, nullptr);
    for (int e = 0; e < c->E; ++e) if (c->owned[e]) nor[e] = c->frames[c->esrc[e]].grid.snor;
    const double* const* d_nor = nullptr;
    MV_CHECK(cached_upload(c, "lin_src_nor", nor.data(), sizeof(void*) * nor.size(), (void**)&d_nor));
    // the low parts of the relative transforms this evaluation uploaded behind the control block (api.cpp upload_rel_sym)
    if (c->sym_lo_dev.cap < sizeof(double) * (size_t)c->E * kEdgeRel) { set_error("%s launch without its relative transforms", what); return MVICP_ERR_STATE; }
    ProfScope ps(c, scope, bytes);
    launch(robust != 0, chunk, (const double*)c->sym_lo_dev.p, d_src, d_nor);
  }
  {
    ProfScope ps(c, "reduce", 0.0);
    hipLaunchKernelGGL((reduce_expand_kernel<true, 1>), dim3(c->E), dim3(256), 0, c->stream, c->d_chunk_first, chunk, c->d_count, c->d_rel, c->d_partials, c->lin_out ? c->lin_out : c->d_out, PairArgs<1>{});
  }
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

}  // namespace

}  // namespace mvicp
