// K5g — the plane-to-plane objective (Segal, Haehnel, Thrun, "Generalized-ICP", RSS 2009) in its standard form: every point carries the covariance
// C(n) = I - (1 - eps) n^ n^T (eps along its normal, 1 in the tangent plane), and the residual vector is weighed by the inverse of the sum of the two.
//
// With the relative transform of linearize_sym.hip (hi + lo, api.cpp upload_rel_sym), a correspondence (p, n_p) of the source frame and (q, n_q) of the dst frame:
//   x' = A p,  p~ = x' + t,  f = p~ - q,  a = n_q,  b = nu = A n_p
//   P(n) = n n^T / (n . n) if n . n is finite and > 0 (as computed in fp64), else 0
//   S = 2 I - (1 - eps) (P(a) + P(b)),  W = 2 eps S^-1                        (symmetric, eigenvalues in [eps, 1]; eps = 1: W = I)
//   s = f^T W f,  J_f = [A, -A [p]x, -I, [p~]x]                                (W frozen at the evaluation poses, fixed in the dst frame)
// For any W = sum_k g_k g_k^T the three rows r_k = g_k . f have the plane family's form u'_k = [g_k ; x' x g_k], u_k = L u'_k, J_k = [Ad^T u_k ; -u_k], and
// share one weight w(s).  Their 28 sums need no factor of W, only W itself: with M = [I ; [x']x] (6 x 3)
//   U = sum w M W M^T = sum w [[W, (x' x W_i)_i], [., x' x (columns of the block above)]]   (21),   v = sum w [W f ; x' x W f]   (6),   cost
// in the plane partial layout, so the per-edge expansion is reduce_expand_kernel<true, 1> (lin_common.h), unchanged.  Loss, corrector, half_rho, the
// scale a = edge.weight and the cost sum rho / 2 are the point family's: soft-L1 on the squared length s of a three-vector; s <= |f|^2.
//
// W without an inverse that cancels.  With a^, b^ the normalised normals (0 for a zero or non-finite one), d = a^ . b^, c = 1 - eps, Woodbury gives
//   W = eps I + kappa [ (1 + eps) (a^ a^T + b^ b^T) + c d (a^ b^T + b^ a^T) ],   kappa = eps c / Delta,
//   Delta = (1 + eps)^2 - c^2 d^2 = 4 eps + c^2 |a^ x b^|^2                     (Lagrange's identity: both terms >= 0, nothing cancels as |d| -> 1)
// and with one of the two normals missing |a^ x b^|^2 is replaced by 1 (Delta = (1 + eps)^2: W = eps I + eps c / (1 + eps) b^ b^T); with both, W = eps I.
// P(n) does not depend on the sign or the length of n: normals are used as stored and their orientation does not matter.
//
// Operation order per correspondence (explicit fma):
//   x'_i, nu_i, f_i, : as linearize_sym.hip (f by residual_component, lin_residual.h)
//   alpha = fma(a2, a2, fma(a1, a1, a0 * a0)),  ok_a = alpha > 0 && alpha < inf,  a^_i = ok_a ? a_i * fast_rsqrt(alpha) : 0;  the same for b
//   d = fma(a^2, b^2, fma(a^1, b^1, a^0 * b^0));  z = a^ x b^ with z_0 = fma(a^1, b^2, -(a^2 * b^1)) and cyclically;  z2 = ok_a && ok_b ? |z|^2 : 1
//   Delta = fma(c * c, z2, 4 eps);  kappa = (eps c) / Delta  (v_rcp_f64 seed + two Newton steps);  k1 = kappa (1 + eps),  k2 = kappa (c d)
//   a'_i = fma(k2, b^_i, k1 * a^_i),  b'_i = fma(k2, a^_i, k1 * b^_i);  W_ij = fma(b^_i, b'_j, fma(a^_i, a'_j, i == j ? eps : 0))  for i <= j
//   y_i = (W f)_i = fma(W_i2, f2, fma(W_i1, f1, W_i0 * f0));  s = fma(f2, y2, fma(f1, y1, f0 * y0))
//   w = 1 (plain) or fast_rsqrt(1 + s * (1 / a^2)),  cost += 0.5 * s or half_rho(s, w)
//   V = w W,  T_i = x' x V_i (row i: T_i0 = fma(x'1, V_i2, -(x'2 * V_i1)) and cyclically),  R_ij = (x' x (T_0j, T_1j, T_2j))_i  for i <= j
//   acc: V (6), T (9), R (6) into the 21 slots of the upper triangle of U, row-major;  v_i += w y_i (3),  v_3.. += x' x (w y) (3)
// then the transposed LDS reduction of linearize_kernel in the same fixed order.
//
// Operands, mapping, look-ahead, chunk tables, XCD interleave, partial slots: those of linearize_sym_kernel, with one difference: the 12 low parts of the
// relative transform are read straight from global memory at a block-uniform address, before the barrier, and so by scalar loads into SGPRs.  Through LDS
// like the high parts they cost 24 VGPRs, and the robust build then needs 256 + 2 AGPRs: one wave per SIMD where this one runs at two (234 / 232 VGPRs).
#include "lin_common.h"
#include "lin_residual.h"

namespace mvicp {

namespace {

// the constants of one launch that depend on eps alone
struct GicpEps { double eps, c, c2, four_eps, eps_c, one_p_eps; };

// n / |n|, or 0 where n . n is zero or not finite; ok says which
__device__ __forceinline__ bool unit_or_zero(double n0, double n1, double n2, double& u0, double& u1, double& u2) {
  const double nn = __builtin_fma(n2, n2, __builtin_fma(n1, n1, n0 * n0));
  const bool ok = nn > 0.0 && nn < __builtin_inf();
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

// One 256-thread workgroup per chunk of one edge, two adjacent correspondences per lane per step, the next step's operands in flight during the
// arithmetic: linearize_sym_kernel's mapping and loads.  Register slots: 0-2 p, 3-5 n_q, 6-8 q, 9-11 n_p.
template <bool ROBUST>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void linearize_gicp_kernel(const int* __restrict__ chunk_edge, const int* __restrict__ chunk_start, int chunk,
                                                            const int* __restrict__ count, const long long* __restrict__ cap_off, long long total_cap,
                                                            const double* __restrict__ rel, const double* __restrict__ rel_lo, const double* __restrict__ a_scale,
                                                            const double* __restrict__ stream, double* __restrict__ partials,
                                                            const double* const* __restrict__ src_pts, const double* const* __restrict__ src_nor,
                                                            const int* __restrict__ first, const int* __restrict__ nsrc,
                                                            const int* __restrict__ chunk_first, double eps) {
  const int e = chunk_edge[blockIdx.x];
  const int start = chunk_start[blockIdx.x];
  const int c = chunk_first[e] + start / chunk;   // the partial's slot: the chunk's place in its edge's run, whatever the launch order
  const int cnt = count[e];
  if (start >= cnt) return;
  const int end = min(cnt, start + chunk);
  // the low parts at a block-uniform address, before the barrier: scalar loads, so they occupy SGPRs, which is what keeps this kernel within 256 VGPRs
  // at two waves per SIMD
  double lo[kEdgeRel];
#pragma unroll
  for (int i = 0; i < kEdgeRel; ++i) lo[i] = rel_lo[(size_t)e * kEdgeRel + i];
  __shared__ double srel[kEdgeRel];
  __shared__ double red[NACC / 2][NT + 1];
  if (threadIdx.x < kEdgeRel) srel[threadIdx.x] = rel[(size_t)e * kEdgeRel + threadIdx.x];
  __syncthreads();
  double A[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) A[i] = srel[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = srel[9 + i];
  double inv_a2 = 1.0;
  if (ROBUST) { const double a = a_scale[e]; inv_a2 = 1.0 / (a * a); }
  GicpEps E;
  E.eps = eps; E.c = 1.0 - eps; E.c2 = E.c * E.c; E.four_eps = 4.0 * eps; E.eps_c = eps * E.c; E.one_p_eps = 1.0 + eps;

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
    accumulate_gicp<ROBUST>(acc, A, t, lo, inv_a2, E, cur[0].x, cur[1].x, cur[2].x, cur[3].x, cur[4].x, cur[5].x, cur[6].x, cur[7].x, cur[8].x, cur[9].x, cur[10].x, cur[11].x);
    if (pos + 1 < end)
      accumulate_gicp<ROBUST>(acc, A, t, lo, inv_a2, E, cur[0].y, cur[1].y, cur[2].y, cur[3].y, cur[4].y, cur[5].y, cur[6].y, cur[7].y, cur[8].y, cur[9].y, cur[10].y, cur[11].y);
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

int launch_linearize_gicp(mvicp_ctx* c, double eps, int robust) {
  if (c->E == 0) return MVICP_OK;
  const int chunk = c->lin_chunk;
  if (c->n_chunks > 0) {
    const double bytes = sym_pass_bytes(c);   // the symmetric pass's bytes: the same operands by the same routes
    // per-edge sorted source clouds and their normals: the symmetric launch's tables (cached by content under the same keys)
    const double* const* d_src = nullptr;
    MV_CHECK(source_table(c, &d_src));
    std::vector<const double*> nor((size_t)c->E, nullptr);
    for (int e = 0; e < c->E; ++e) if (c->owned[e]) nor[e] = c->frames[c->esrc[e]].grid.snor;
    const double* const* d_nor = nullptr;
    MV_CHECK(cached_upload(c, "lin_src_nor", nor.data(), sizeof(void*) * nor.size(), (void**)&d_nor));
    // the low parts of the relative transforms this evaluation uploaded behind the control block (api.cpp upload_rel_sym)
    if (c->sym_lo_dev.cap < sizeof(double) * (size_t)c->E * kEdgeRel) { set_error("gicp launch without its relative transforms"); return MVICP_ERR_STATE; }
    const double* d_lo = (const double*)c->sym_lo_dev.p;
    ProfScope ps(c, "linearize_gicp", bytes);
#define LAUNCH(R)                                                                                                                               \
  hipLaunchKernelGGL((linearize_gicp_kernel<R>), dim3(c->n_chunks), dim3(NT), 0, c->stream, c->d_chunk_edge, c->d_chunk_start, chunk, c->d_count, \
                     c->d_cap_off, c->total_cap, c->d_rel, d_lo, c->d_a, c->d_stream, c->d_partials, d_src, d_nor, (const int*)c->d_first,       \
                     (const int*)c->d_nsrc, (const int*)c->d_chunk_first, eps)
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
