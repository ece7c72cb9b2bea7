// K5g — the plane-to-plane objective (Segal, Haehnel, Thrun, "Generalized-ICP", RSS 2009) in its standard form: every point carries the covariance
// C(n) = I - (1 - eps) n^ n^T (eps along its normal, 1 in the tangent plane), and the residual vector is weighed by the inverse of the sum of the two.
//
// With the relative transform of linearize_sym.hip (hi + lo, api.cpp upload_rel_sym), a correspondence (p, n_p) of the source frame and (q, n_q) of the dst frame:
//   x' = A p,  p~ = x' + t,  f = p~ - q,  a = n_q,  b = nu = A n_p
//   P(n) = n n^T / (n . n) if 2^-1022 <= n . n < inf (as computed in fp64: a normal number), else 0
//   S = 2 I - (1 - eps) (P(a) + P(b)),  W = 2 eps S^-1                        (symmetric, eigenvalues in [eps, 1]; eps = 1: W = I)
//   s = f^T W f,  J_f = [A, -A [p]x, -I, [p~]x]                                (W frozen at the evaluation poses, fixed in the dst frame)
// For any W = sum_k g_k g_k^T the three rows r_k = g_k . f have the plane family's form u'_k = [g_k ; x' x g_k], u_k = L u'_k, J_k = [Ad^T u_k ; -u_k], and
// share one weight w(s).  Their 28 sums need no factor of W, only W itself: with M = [I ; [x']x] (6 x 3)
//   U = sum w M W M^T = sum w [[W, (x' x W_i)_i], [., x' x (columns of the block above)]]   (21),   v = sum w [W f ; x' x W f]   (6),   cost
// in the plane partial layout, so the per-edge expansion is reduce_expand_kernel<true, 1> (lin_common.h), unchanged.  Loss, corrector, half_rho, the
// scale a = edge.weight and the cost sum rho / 2 are the point family's: soft-L1 on the squared length s of a three-vector; s <= |f|^2.
//
// W without an inverse that cancels.  With a^, b^ the normalised normals (0 where P(n) = 0), d = a^ . b^, c = 1 - eps, Woodbury gives
//   W = eps I + kappa [ (1 + eps) (a^ a^T + b^ b^T) + c d (a^ b^T + b^ a^T) ],   kappa = eps c / Delta,
//   Delta = (1 + eps)^2 - c^2 d^2 = 4 eps + c^2 |a^ x b^|^2                     (Lagrange's identity: both terms >= 0, nothing cancels as |d| -> 1)
// and with one of the two normals missing |a^ x b^|^2 is replaced by 1 (Delta = (1 + eps)^2: W = eps I + eps c / (1 + eps) b^ b^T); with both, W = eps I.
// P(n) does not depend on the sign or the length of n: normals are used as stored and their orientation does not matter.
//
// Operation order per correspondence (explicit fma):
//   x'_i, nu_i, f_i, : as linearize_sym.hip (f by residual_component, lin_residual.h)
//   alpha = fma(a2, a2, fma(a1, a1, a0 * a0)),  ok_a = alpha >= 2^-1022 && alpha < inf,  a^_i = ok_a ? a_i * fast_rsqrt(alpha) : 0;  the same for b
//   d = fma(a^2, b^2, fma(a^1, b^1, a^0 * b^0));  z = a^ x b^ with z_0 = fma(a^1, b^2, -(a^2 * b^1)) and cyclically;  z2 = ok_a && ok_b ? |z|^2 : 1
//   Delta = fma(c * c, z2, 4 eps);  kappa = (eps c) / Delta  (v_rcp_f64 seed + two Newton steps);  k1 = kappa (1 + eps),  k2 = kappa (c d)
//   a'_i = fma(k2, b^_i, k1 * a^_i),  b'_i = fma(k2, a^_i, k1 * b^_i);  W_ij = fma(b^_i, b'_j, fma(a^_i, a'_j, i == j ? eps : 0))  for i <= j
//   y_i = (W f)_i = fma(W_i2, f2, fma(W_i1, f1, W_i0 * f0));  s = fma(f2, y2, fma(f1, y1, f0 * y0))
//   w = 1 (plain) or fast_rsqrt(1 + s * (1 / a^2)),  cost += 0.5 * s or half_rho(s, w)
//   V = w W,  T_i = x' x V_i (row i: T_i0 = fma(x'1, V_i2, -(x'2 * V_i1)) and cyclically),  R_ij = (x' x (T_0j, T_1j, T_2j))_i  for i <= j
//   acc: V (6), T (9), R (6) into the 21 slots of the upper triangle of U, row-major;  v_i += w y_i (3),  v_3.. += x' x (w y) (3)
// then the block reduction of every family (block_reduce_store, lin_common.h).
//
// Operands, mapping, look-ahead, chunk tables, XCD interleave, partial slots and the host launch: lin_normal.h, shared with the symmetric objective
// (linearize_sym.hip), with its switch set to the scalar route for the 12 low parts of the relative transform (see the kernel below).
#include "lin_normal.h"
#include "lin_residual.h"

namespace mvicp {

namespace {

// the constants of one launch that depend on eps alone
struct GicpEps { double eps, c, c2, four_eps, eps_c, one_p_eps; };

// n / |n|, or 0 where n . n is below 2^-1022 (zero or subnormal: it no longer carries the length of n) or not finite; ok says which.
// fast_rsqrt (documented for y >= 1) is used on [2^-1022, inf): y r r stays of order 1 there, and r r <= 2^1022 does not overflow.
__device__ __forceinline__ bool unit_or_zero(double n0, double n1, double n2, double& u0, double& u1, double& u2) {
  const double nn = __builtin_fma(n2, n2, __builtin_fma(n1, n1, n0 * n0));
  const bool ok = nn >= 0x1p-1022 && nn < __builtin_inf();
  const double r = fast_rsqrt(ok ? nn : 1.0);
  u0 = ok ? n0 * r : 0.0; u1 = ok ? n1 * r : 0.0; u2 = ok ? n2 * r : 0.0;
  return ok;
}

template <bool ROBUST>
__device__ __forceinline__ void accumulate_gicp(double (&acc)[NACC], const double* __restrict__ A, const double* __restrict__ t, const double* __restrict__ lo, double inv_a2,
                                                const GicpEps& E, double p0, double p1, double p2, double n0, double n1, double n2, double q0, double q1, double q2,
                                                double s0, double s1, double s2) {
#pragma clang fp contract(off)   // every fma of this function is written out: the sums into acc add values that were rounded once
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
  double a0, a1, a2, b0, b1, b2;
  const bool ok_a = unit_or_zero(n0, n1, n2, a0, a1, a2);
  const bool ok_b = unit_or_zero(v0, v1, v2, b0, b1, b2);
  const double d = __builtin_fma(a2, b2, __builtin_fma(a1, b1, a0 * b0));
  const double z0 = __builtin_fma(a1, b2, -(a2 * b1)), z1 = __builtin_fma(a2, b0, -(a0 * b2)), z2 = __builtin_fma(a0, b1, -(a1 * b0));
  const double zz = (ok_a && ok_b) ? __builtin_fma(z2, z2, __builtin_fma(z1, z1, z0 * z0)) : 1.0;
  const double delta = __builtin_fma(E.c2, zz, E.four_eps);   // in [4 eps, (1 + eps)^2]
  double rd = __builtin_amdgcn_rcp(delta);
  rd = __builtin_fma(__builtin_fma(-delta, rd, 1.0), rd, rd);
  rd = __builtin_fma(__builtin_fma(-delta, rd, 1.0), rd, rd);
  const double kappa = E.eps_c * rd;
  const double k1 = kappa * E.one_p_eps, k2 = kappa * (E.c * d);
  const double aa0 = __builtin_fma(k2, b0, k1 * a0), aa1 = __builtin_fma(k2, b1, k1 * a1), aa2 = __builtin_fma(k2, b2, k1 * a2);
  const double bb0 = __builtin_fma(k2, a0, k1 * b0), bb1 = __builtin_fma(k2, a1, k1 * b1), bb2 = __builtin_fma(k2, a2, k1 * b2);
  // W, upper triangle: 00 01 02 11 12 22
  const double W00 = __builtin_fma(b0, bb0, __builtin_fma(a0, aa0, E.eps)), W01 = __builtin_fma(b0, bb1, a0 * aa1), W02 = __builtin_fma(b0, bb2, a0 * aa2);
  const double W11 = __builtin_fma(b1, bb1, __builtin_fma(a1, aa1, E.eps)), W12 = __builtin_fma(b1, bb2, a1 * aa2);
  const double W22 = __builtin_fma(b2, bb2, __builtin_fma(a2, aa2, E.eps));
  const double y0 = __builtin_fma(W02, f2, __builtin_fma(W01, f1, W00 * f0));
  const double y1 = __builtin_fma(W12, f2, __builtin_fma(W11, f1, W01 * f0));
  const double y2 = __builtin_fma(W22, f2, __builtin_fma(W12, f1, W02 * f0));
  const double s = __builtin_fma(f2, y2, __builtin_fma(f1, y1, f0 * y0));
  double w = 1.0;
  if (ROBUST) {
    const double y = 1.0 + s * inv_a2;
    w = fast_rsqrt(y);
    acc[27] += half_rho(s, w);
  } else {
    acc[27] += 0.5 * s;
  }
  // V = w W, rows V[i][.] (symmetric); T[i][k] = (x' x V_i)_k; R[i][j] = (x' x T_.j)_i
  const double V[3][3] = {{w * W00, w * W01, w * W02}, {w * W01, w * W11, w * W12}, {w * W02, w * W12, w * W22}};
  const double x[3] = {x0, x1, x2};
  double T[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    T[i][0] = __builtin_fma(x[1], V[i][2], -(x[2] * V[i][1]));
    T[i][1] = __builtin_fma(x[2], V[i][0], -(x[0] * V[i][2]));
    T[i][2] = __builtin_fma(x[0], V[i][1], -(x[1] * V[i][0]));
  }
  // upper triangle of U, row-major over 6 x 6: rows 0-2 = [V_i(i..2) | T_i(0..2)], rows 3-5 = R_i(i..2)
  int o = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = i; j < 3; ++j) { acc[o] += V[i][j]; ++o; }
#pragma unroll
    for (int j = 0; j < 3; ++j) { acc[o] += T[i][j]; ++o; }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
    for (int j = i; j < 3; ++j) { acc[o] += __builtin_fma(x[i1], T[i2][j], -(x[i2] * T[i1][j])); ++o; }
  }
  const double wy0 = w * y0, wy1 = w * y1, wy2 = w * y2;
  acc[21] += wy0; acc[22] += wy1; acc[23] += wy2;
  acc[24] += __builtin_fma(x1, wy2, -(x2 * wy1));
  acc[25] += __builtin_fma(x2, wy0, -(x0 * wy2));
  acc[26] += __builtin_fma(x0, wy1, -(x1 * wy0));
}

// The shared pipeline (lin_normal.h) around accumulate_gicp, the 12 low parts by scalar loads: through LDS like the high parts they cost 24 VGPRs, and
// the robust build then needs 256 + 2 AGPRs: one wave per SIMD where this one runs at two (234 / 232 VGPRs).
template <bool ROBUST>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void linearize_gicp_kernel(const int* __restrict__ chunk_edge, const int* __restrict__ chunk_start, int chunk,
                                                            const int* __restrict__ count, const long long* __restrict__ cap_off, long long total_cap,
                                                            const double* __restrict__ rel, const double* __restrict__ rel_lo, const double* __restrict__ a_scale,
                                                            const double* __restrict__ stream, double* __restrict__ partials,
                                                            const double* const* __restrict__ src_pts, const double* const* __restrict__ src_nor,
                                                            const int* __restrict__ first, const int* __restrict__ nsrc,
                                                            const int* __restrict__ chunk_first, double eps) {
  GicpEps E;
  E.eps = eps; E.c = 1.0 - eps; E.c2 = E.c * E.c; E.four_eps = 4.0 * eps; E.eps_c = eps * E.c; E.one_p_eps = 1.0 + eps;
  linearize_normal_body<ROBUST, true>(chunk_edge, chunk_start, chunk, count, cap_off, total_cap, rel, rel_lo, a_scale, stream, partials, src_pts, src_nor, first, nsrc, chunk_first,
                                      [&E](double (&acc)[NACC], const double* A, const double* t, const double* lo, double inv_a2, auto... operands) {
                                        accumulate_gicp<ROBUST>(acc, A, t, lo, inv_a2, E, operands...);
                                      });
}

}  // namespace

// (the symmetric launch's tables, cached by content under the same keys, and the symmetric pass's bytes: the same operands by the same routes)
int launch_linearize_gicp(mvicp_ctx* c, double eps, int robust) {
  return launch_linearize_normal(c, robust, "linearize_gicp", "gicp", [&](bool rob, int chunk, const double* d_lo, const double* const* d_src, const double* const* d_nor) {
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(c->n_lin_wg), dim3(NT), 0, c->stream, c->d_chunk_edge, c->d_chunk_start, chunk, c->d_count, c->d_cap_off, c->total_cap, c->d_rel, d_lo,
                         c->d_a, c->d_stream, c->d_partials, d_src, d_nor, (const int*)c->d_first, (const int*)c->d_nsrc, (const int*)c->d_chunk_first, eps);
    };
    if (rob) go(linearize_gicp_kernel<true>);
    else go(linearize_gicp_kernel<false>);
  });
}

}  // namespace mvicp
