// K5s — the symmetric point-to-plane objective (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019): the residual uses the MEAN of
// the two normals, so it vanishes at the true pose wherever the surface is locally quadratic between the two samples, where the point-to-plane residual
// n_q . (p~ - q) keeps a bias of the size of the curvature times the sample distance squared.
//
// With the relative transform of linearize.hip, A = R_d^T R_s, t = R_d^T (t_s - t_d), a correspondence (p, n_p) of the source frame and (q, n_q) of the dst frame:
//   x' = A p,  p~ = x' + t,  nu = A n_p,  m = (n_q + nu) / 2,  f = p~ - q
//   r  = m . f
//   u  = [ m ; (p~ x n_q + q x nu) / 2 ],          J = [ Ad^T u ; -u ]      (coordinates [ups_s, om_s, ups_d, om_d], T <- T exp(delta))
//   u' = [ m ; (x' x n_q + (q - t) x nu) / 2 ],    u = L u',  L = [[I, 0], [[t]x, I]]     (moments about t, as in linearize.hip)
// so the per-lane sums are the plane family's 28 (U = sum w u' u'^T (21), v = sum w r u' (6), cost), the partial layout is the plane one, and the per-edge
// expansion is reduce_expand_kernel<true, 1> (lin_common.h), unchanged.  Loss, corrector, half_rho, the scale a = edge.weight and the cost sum rho / 2 are the
// plane family's.  The factor 1/2 makes r the point-to-plane residual when the two normals agree, so the robust scale and last_rms keep their meaning.
// Normals are used AS STORED: no sign flip, no normalisation.  Orienting the normals of the two clouds consistently (n_p . A^T n_q > 0 for matching points)
// is the caller's job; with opposite orientations m is the half DIFFERENCE of the normals and the objective is meaningless.
//
// Operation order per correspondence (explicit fma, one rounding sequence whatever the compiler's contraction rules):
//   x'_i  = fma(A[i+6], p2, fma(A[i+3], p1, A[i] * p0))          (A column-major; as accumulate<> in linearize.hip)
//   nu_i  = fma(A[i+6], s2, fma(A[i+3], s1, A[i] * s0))          (s = n_p)
//   m_i   = 0.5 * (n_i + nu_i)                                   (n = n_q)
//   f_i   = residual_component() (lin_residual.h): h_k = A[i+3k] * p_k with its exact error g_k = fma(A[i+3k], p_k, -h_k); TwoSum chain s1 = h_0 + h_1, s2 = s1 + h_2, s3 = s2 + t_i,
//           s4 = s3 - q_i with errors e1..e4;  f_i = s4 + ((((e1 + e2) + (e3 + e4)) + ((g_0 + g_1) + g_2)) + fma(Alo[i+6], p2, fma(Alo[i+3], p1, fma(Alo[i], p0, tlo_i))))
//   d_i   = q_i - t_i
//   r     = fma(m2, f2, fma(m1, f1, m0 * f0))
//   u'_3  = 0.5 * fma(x'1, n2, fma(-x'2, n1, fma(d1, nu2, -(d2 * nu1))))     and cyclically (1,2) -> (2,0) -> (0,1) for u'_4, u'_5
//   s = r * r,  w = 1 (plain) or fast_rsqrt(1 + s * (1 / a^2)),  cost += 0.5 * s or half_rho(s, w)
//   for i = 0..5: wu = w * u'_i;  U_ij = fma(wu, u'_j, U_ij) for j = i..5;  v_i = fma(wu, r, v_i)
// then the transposed LDS reduction of linearize_kernel in the same fixed order.
//
// The relative transform comes as hi + lo (api.cpp upload_rel_sym: R_d^-1 by the true inverse, in extended precision): an error of (A, t) is common to
// every correspondence of the edge and would add up coherently in g against residuals that add up like sqrt(N).  The low parts enter the residual's f
// only; the moments, nu and the expansion use the hi parts, where that error is an ordinary relative one.
//
// Operands: n_q (arrays 3-5) and q (arrays 7-9) from the operand stream, non-temporal; p from arrays 0-2 or, for an identity list, from the shared
// sorted source cloud (as linearize_kernel); n_p from the source frame's sorted normals at first[pos] — the stream is NOT widened — which for an identity
// list is position pos itself, three 16-B loads per pair like p.  Both cloud-side loads are ordinary cacheable loads: the edges of a source frame share them.
// The gather index of the step AFTER the next is loaded one step early, so its latency is not on the path of the prefetch that depends on it.
// Mapping, chunk tables, partial slots: those of linearize_kernel (launch_linearize's tables; the XCD interleave comes with them).
#include "lin_common.h"
#include "lin_residual.h"

namespace mvicp {

namespace {

template <bool ROBUST>
__device__ __forceinline__ void accumulate_sym(double (&acc)[NACC], const double* __restrict__ A, const double* __restrict__ t, const double* __restrict__ lo, double inv_a2,
                                               double p0, double p1, double p2, double n0, double n1, double n2, double q0, double q1, double q2,
                                               double s0, double s1, double s2) {
  const double x0 = __builtin_fma(A[6], p2, __builtin_fma(A[3], p1, A[0] * p0));
  const double x1 = __builtin_fma(A[7], p2, __builtin_fma(A[4], p1, A[1] * p0));
  const double x2 = __builtin_fma(A[8], p2, __builtin_fma(A[5], p1, A[2] * p0));
  const double v0 = __builtin_fma(A[6], s2, __builtin_fma(A[3], s1, A[0] * s0));
  const double v1 = __builtin_fma(A[7], s2, __builtin_fma(A[4], s1, A[1] * s0));
  const double v2 = __builtin_fma(A[8], s2, __builtin_fma(A[5], s1, A[2] * s0));
  // (lo[0..8] = A's low parts, lo[9..11] = t's)
  const double f0 = residual_component(A[0], A[3], A[6], t[0], p0, p1, p2, q0, __builtin_fma(lo[6], p2, __builtin_fma(lo[3], p1, __builtin_fma(lo[0], p0, lo[9]))));
  const double f1 = residual_component(A[1], A[4], A[7], t[1], p0, p1, p2, q1, __builtin_fma(lo[7], p2, __builtin_fma(lo[4], p1, __builtin_fma(lo[1], p0, lo[10]))));
  const double f2 = residual_component(A[2], A[5], A[8], t[2], p0, p1, p2, q2, __builtin_fma(lo[8], p2, __builtin_fma(lo[5], p1, __builtin_fma(lo[2], p0, lo[11]))));
  const double d0 = q0 - t[0], d1 = q1 - t[1], d2 = q2 - t[2];
  double u[6];
  u[0] = 0.5 * (n0 + v0); u[1] = 0.5 * (n1 + v1); u[2] = 0.5 * (n2 + v2);
  u[3] = 0.5 * __builtin_fma(x1, n2, __builtin_fma(-x2, n1, __builtin_fma(d1, v2, -(d2 * v1))));
  u[4] = 0.5 * __builtin_fma(x2, n0, __builtin_fma(-x0, n2, __builtin_fma(d2, v0, -(d0 * v2))));
  u[5] = 0.5 * __builtin_fma(x0, n1, __builtin_fma(-x1, n0, __builtin_fma(d0, v1, -(d1 * v0))));
  const double r = __builtin_fma(u[2], f2, __builtin_fma(u[1], f1, u[0] * f0));
  const double s = r * r;
  double w = 1.0;
  if (ROBUST) {
    const double y = 1.0 + s * inv_a2;
    w = fast_rsqrt(y);
    acc[27] += half_rho(s, w);
  } else {
    acc[27] += 0.5 * s;
  }
  int o = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double wu = w * u[i];
#pragma unroll
    for (int j = i; j < 6; ++j) { acc[o] = __builtin_fma(wu, u[j], acc[o]); ++o; }
    acc[21 + i] = __builtin_fma(wu, r, acc[21 + i]);
  }
}

// One 256-thread workgroup per chunk of one edge, two adjacent correspondences per lane per step, the next step's operands in flight during the
// arithmetic: linearize_kernel's mapping.  Register slots: 0-2 p, 3-5 n_q, 6-8 q, 9-11 n_p.
template <bool ROBUST>
__global__ __launch_bounds__(NT) void linearize_sym_kernel(const int* __restrict__ chunk_edge, const int* __restrict__ chunk_start, int chunk,
                                                           const int* __restrict__ count, const long long* __restrict__ cap_off, long long total_cap,
                                                           const double* __restrict__ rel, const double* __restrict__ rel_lo, const double* __restrict__ a_scale,
                                                           const double* __restrict__ stream, double* __restrict__ partials,
                                                           const double* const* __restrict__ src_pts, const double* const* __restrict__ src_nor,
                                                           const int* __restrict__ first, const int* __restrict__ nsrc,
                                                           const int* __restrict__ chunk_first) {
  const int e = chunk_edge[blockIdx.x];
  const int start = chunk_start[blockIdx.x];
  const int c = chunk_first[e] + start / chunk;   // the partial's slot: the chunk's place in its edge's run, whatever the launch order
  const int cnt = count[e];
  if (start >= cnt) return;
  const int end = min(cnt, start + chunk);
  __shared__ double srel[2][kEdgeRel];
  __shared__ double red[NACC / 2][NT + 1];
  if (threadIdx.x < kEdgeRel) srel[0][threadIdx.x] = rel[(size_t)e * kEdgeRel + threadIdx.x];
  if (threadIdx.x >= 32 && threadIdx.x < 32 + kEdgeRel) srel[1][threadIdx.x - 32] = rel_lo[(size_t)e * kEdgeRel + threadIdx.x - 32];
  __syncthreads();
  double A[9], t[3], lo[kEdgeRel];
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] = srel[0][i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = srel[0][9 + i];
#pragma unroll
  for (int i = 0; i < kEdgeRel; ++i) lo[i] = srel[1][i];
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
    accumulate_sym<ROBUST>(acc, A, t, lo, inv_a2, cur[0].x, cur[1].x, cur[2].x, cur[3].x, cur[4].x, cur[5].x, cur[6].x, cur[7].x, cur[8].x, cur[9].x, cur[10].x, cur[11].x);
    if (pos + 1 < end)
      accumulate_sym<ROBUST>(acc, A, t, lo, inv_a2, cur[0].y, cur[1].y, cur[2].y, cur[3].y, cur[4].y, cur[5].y, cur[6].y, cur[7].y, cur[8].y, cur[9].y, cur[10].y, cur[11].y);
#pragma unroll
    for (int j = 0; j < NS; ++j) cur[j] = nxt[j];
    pos = npos;
  }

  // Block reduction through LDS, transposed, in the fixed order of linearize_kernel: row j holds value j of every lane, 16 threads per row add 16 columns
  // each and finish with a 4-step xor-shuffle; two passes of 16 rows.
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) __syncthreads();
#pragma unroll
    for (int j = 0; j < NACC / 2; ++j) red[j][threadIdx.x] = acc[pass * (NACC / 2) + j];
    __syncthreads();
    const int row = threadIdx.x >> 4, part = threadIdx.x & 15;
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < NT / 16; ++i) sum += red[row][part + 16 * i];
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    sum += __shfl_xor(sum, 8, 64);
    if (part == 0) partials[(size_t)c * NACC + pass * (NACC / 2) + row] = sum;
  }
}

}  // namespace

int launch_linearize_sym(mvicp_ctx* c, int robust) {
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
    if (c->sym_lo_dev.cap < sizeof(double) * (size_t)c->E * kEdgeRel) { set_error("symmetric launch without its relative transforms"); return MVICP_ERR_STATE; }
    const double* d_lo = (const double*)c->sym_lo_dev.p;
    ProfScope ps(c, "linearize_sym", bytes);
#define LAUNCH(R)                                                                                                                              \
  hipLaunchKernelGGL((linearize_sym_kernel<R>), dim3(c->n_chunks), dim3(NT), 0, c->stream, c->d_chunk_edge, c->d_chunk_start, chunk, c->d_count, \
                     c->d_cap_off, c->total_cap, c->d_rel, d_lo, c->d_a, c->d_stream, c->d_partials, d_src, d_nor, (const int*)c->d_first,      \
                     (const int*)c->d_nsrc, (const int*)c->d_chunk_first)
    if (robust) LAUNCH(true);
    else LAUNCH(false);
#undef LAUNCH
  }
  {
    ProfScope ps(c, "reduce", 0.0);
    hipLaunchKernelGGL((reduce_expand_kernel<true, 1>), dim3(c->E), dim3(256), 0, c->stream, c->d_chunk_first, chunk, c->d_count, c->d_rel, c->d_partials, c->lin_out ? c->lin_out : c->d_out, PairArgs<1>{});
  }
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

}  // namespace mvicp
