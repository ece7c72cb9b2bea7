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
// then the block reduction of every family (block_reduce_store, lin_common.h).
//
// The relative transform comes as hi + lo (api.cpp upload_rel_sym: R_d^-1 by the true inverse, in extended precision): an error of (A, t) is common to
// every correspondence of the edge and would add up coherently in g against residuals that add up like sqrt(N).  The low parts enter the residual's f
// only; the moments, nu and the expansion use the hi parts, where that error is an ordinary relative one.
//
// Operands, mapping, look-ahead, chunk tables, XCD interleave, partial slots and the host launch: lin_normal.h, shared with the plane-to-plane objective
// (linearize_gicp.hip).  This file holds the arithmetic of one correspondence; the 12 low parts reach it through LDS, next to the high parts.
#include "lin_normal.h"
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

// The shared pipeline (lin_normal.h) around accumulate_sym, the 12 low parts through LDS.
template <bool ROBUST>
__global__ __launch_bounds__(NT) void linearize_sym_kernel(const int* __restrict__ chunk_edge, const int* __restrict__ chunk_start, int chunk,
                                                           const int* __restrict__ count, const long long* __restrict__ cap_off, long long total_cap,
                                                           const double* __restrict__ rel, const double* __restrict__ rel_lo, const double* __restrict__ a_scale,
                                                           const double* __restrict__ stream, double* __restrict__ partials,
                                                           const double* const* __restrict__ src_pts, const double* const* __restrict__ src_nor,
                                                           const int* __restrict__ first, const int* __restrict__ nsrc,
                                                           const int* __restrict__ chunk_first) {
  linearize_normal_body<ROBUST, false>(chunk_edge, chunk_start, chunk, count, cap_off, total_cap, rel, rel_lo, a_scale, stream, partials, src_pts, src_nor, first, nsrc, chunk_first,
                                       [](double (&acc)[NACC], auto... operands) { accumulate_sym<ROBUST>(acc, operands...); });
}

}  // namespace

int launch_linearize_sym(mvicp_ctx* c, int robust) {
  return launch_linearize_normal(c, robust, "linearize_sym", "symmetric", [&](bool rob, int chunk, const double* d_lo, const double* const* d_src, const double* const* d_nor) {
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(c->n_lin_wg), dim3(NT), 0, c->stream, c->d_chunk_edge, c->d_chunk_start, chunk, c->d_count, c->d_cap_off, c->total_cap, c->d_rel, d_lo,
                         c->d_a, c->d_stream, c->d_partials, d_src, d_nor, (const int*)c->d_first, (const int*)c->d_nsrc, (const int*)c->d_chunk_first);
    };
    if (rob) go(linearize_sym_kernel<true>);
    else go(linearize_sym_kernel<false>);
  });
}

}  // namespace mvicp
