// K5 — per-correspondence residual + analytic SE(3) Jacobian, robust weighting, block-reduced
// J^T J / J^T r / cost per edge.  HBM-bandwidth bound: each LM evaluation streams the packed operand
// stream once (56 B / correspondence point-to-plane, 48 B point-to-point), fully coalesced.
//
// Operand stream (SoA, `total_cap` doubles per array, written once per round by the gather kernel, corr.hip):
//   arrays 0-2 p (source point, src frame) | 3-5 n (dst normal) | 6 c = n . q | 7-9 q (dst point).
// Point-to-plane needs q only through the scalar c:  r = n . (p~ - q) = n . p~ - c,  so it reads 7 arrays instead
// of 9 (-22 % bytes on the kernel that dominates the LM phase).  The two forms of r differ by the rounding of O(|p~|)-sized dot products: an absolute
// error of a few eps |p~| per residual, which the assembled g carries as ~eps |p~| / |r| RELATIVE — 1e-14 for unit-scale clouds with mm residuals, but
// growing in proportion to the distance of the data from the dst frame's origin (1e-10 at |p~| = 1e4).  An fp64 evaluation of the reference's own
// functors rounds p~ the same way and loses the same digits (families "t" and "W"); H and the cost are not affected.
//
// Replaces what Ceres does with one AutoDiffCostFunction + SoftLOneLoss per correspondence
// (src/internal/icp-ceres.cpp:270-292,360-378,435-453 on the functors of include/icp-ceres.h:49-316):
// evaluate r and dr/d(pose_s, pose_d), scale both by sqrt(rho') (Ceres corrector for rho'' <= 0), and
// accumulate the normal equations, in canonical right-perturbation coordinates T <- T exp([upsilon, omega])
// for both poses (the host LM maps them to the selected parameterization, host/lm.cpp).
//
// Structure exploited (docs/mv-lm-icp.tex:109-112,306-319).  With the RELATIVE transform
//   A = R_d^T R_s,  t = R_d^T (t_s - t_d),  p~ = A p + t  (source point in the dst frame),
// and Ad = [[A, [t]x A], [0, A]] its adjoint, every Jacobian row is a fixed linear image of a 6-vector
// that lives in the dst frame:
//   point-to-plane  r = n . (p~ - q),  u = [n ; p~ x n],           J = [ Ad^T u ; -u ]
//   point-to-point  r = p~ - q,        u_k = [e_k ; p~ x e_k],     J_k = [ Ad^T u_k ; -u_k + [0 ; r x e_k] ]
// so instead of 78 + 12 + 1 running sums per lane only a weighted 6x6 moment block is accumulated.
//
// CENTRED MOMENTS.  Moments of u itself are of size |p~|^2, while the source-side Jacobian [A^T n ; p x A^T n] is of size |p|: when t is large
// against the spread of the source cloud (views expressed in displaced sensor frames), Ad^T U Ad cancels and H_ss loses (|t| / spread)^2 eps.
// So the moments are taken about t:  x' = A p (rotated, not translated),  u' = [n ; x' x n]  resp.  u'_k = [e_k ; x' x e_k].  Then
//   u = L u',  L = [[I, 0], [[t]x, I]],  and  Ad^T L = diag(A^T, A^T) =: R6^T,  L [0 ; z] = [0 ; z],
// and nothing in the expansion cancels.  Accumulated per lane:
//   plane (28 sums):  U = sum w u' u'^T (21), v = sum w r u' (6), cost
//   point (29 sums):  sum w {1, x' (3), x' x'^T (6), r (3), x' r^T (9), r r^T (6)}, cost
// with r from p~ = x' + t (plane: r = n . x' + (n . t - c)), w = rho'(|r|^2) = 1/sqrt(1 + |r|^2 / a^2), cost = sum rho/2,
// rho = 2 a^2 (sqrt(1 + s/a^2) - 1) (ceres::SoftLOneLoss(a = edge.weight) [upstream]; evaluated as 2 s w / (1 + w), half_rho below), and the 12x12 block is expanded ONCE per edge:
//   H_ss = R6^T S R6, H_sd = -R6^T (S - X) L^T, H_dd = L (S - X - X^T + Y) L^T, g = [R6^T v ; -L v]
//   (plane: S = U, X = Y = 0; point: S = sum w [[I, -[x']x],[[x']x, -[x']x^2]], X = sum w [[0,-[r]x],[0,-[x']x[r]x]],
//    Y = sum w [[0,0],[0,-[r]x^2]], v = sum w [r ; x' x r]).
//
// Mapping: one 256-thread workgroup per chunk of `chunk` correspondences of ONE edge; ~60 accumulator
// VGPRs per lane leave room to keep the next correspondences' loads in flight; transposed LDS block
// reduction (block_reduce_store, lin_common.h: one text for every family); one partial per workgroup; a second kernel sums each edge's partials in fixed order and does
// the expansion -> deterministic, and independent of how edges are sharded across GPUs.
#include "lin_common.h"

namespace mvicp {

namespace {

template <bool PLANE, bool ROBUST>
__device__ __forceinline__ void accumulate(double (&acc)[NACC], const double* __restrict__ A, const double* __restrict__ t, double inv_a2,
                                           double p0, double p1, double p2, double q0, double q1, double q2, double n0, double n1, double n2) {
  // PLANE: (q0, q1, q2) = (c, -, -) with c = n . q;  POINT: (n0, n1, n2) unused
  // x' = A p: the source point rotated into the dst frame but NOT translated — the moments are taken about the relative translation t (see the header);
  // only the residual sees p~ = x' + t.  Explicit fma throughout: one rounding sequence whatever the build (one or two pose sets).
  const double x0 = __builtin_fma(A[6], p2, __builtin_fma(A[3], p1, A[0] * p0));
  const double x1 = __builtin_fma(A[7], p2, __builtin_fma(A[4], p1, A[1] * p0));
  const double x2 = __builtin_fma(A[8], p2, __builtin_fma(A[5], p1, A[2] * p0));
  if (PLANE) {
    // r = n . x' + (n . t - c)
    const double nt_c = __builtin_fma(n2, t[2], __builtin_fma(n1, t[1], __builtin_fma(n0, t[0], -q0)));
    const double r = __builtin_fma(n2, x2, __builtin_fma(n1, x1, n0 * x0)) + nt_c;
    double u[6];
    u[0] = n0; u[1] = n1; u[2] = n2;
    u[3] = x1 * n2 - x2 * n1; u[4] = x2 * n0 - x0 * n2; u[5] = x0 * n1 - x1 * n0;
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
      // (explicit fma: what the compiler contracts these to anyway; spelled out so that the two-pose build, where n_i n_j is common to both pose sets
      // when w = 1, cannot keep the shared product as a separate rounded multiply)
      for (int j = i; j < 6; ++j) { acc[o] = __builtin_fma(wu, u[j], acc[o]); ++o; }
      acc[21 + i] = __builtin_fma(wu, r, acc[21 + i]);
    }
  } else {
    const double f0 = (x0 + t[0]) - q0, f1 = (x1 + t[1]) - q1, f2 = (x2 + t[2]) - q2;   // r = p~ - q, p~ = x' + t
    const double s = f0 * f0 + f1 * f1 + f2 * f2;
    double w = 1.0;
    if (ROBUST) {
      const double y = 1.0 + s * inv_a2;
      w = fast_rsqrt(y);
      acc[28] += half_rho(s, w);
    } else {
      acc[28] += 0.5 * s;
    }
    const double wx0 = w * x0, wx1 = w * x1, wx2 = w * x2;
    const double wf0 = w * f0, wf1 = w * f1, wf2 = w * f2;
    acc[0] += w;
    acc[1] += wx0; acc[2] += wx1; acc[3] += wx2;
    acc[4] += wx0 * x0; acc[5] += wx0 * x1; acc[6] += wx0 * x2; acc[7] += wx1 * x1; acc[8] += wx1 * x2; acc[9] += wx2 * x2;
    acc[10] += wf0; acc[11] += wf1; acc[12] += wf2;
    acc[13] += wx0 * f0; acc[14] += wx0 * f1; acc[15] += wx0 * f2;
    acc[16] += wx1 * f0; acc[17] += wx1 * f1; acc[18] += wx1 * f2;
    acc[19] += wx2 * f0; acc[20] += wx2 * f1; acc[21] += wx2 * f2;
    acc[22] += wf0 * f0; acc[23] += wf0 * f1; acc[24] += wf0 * f2; acc[25] += wf1 * f1; acc[26] += wf1 * f2; acc[27] += wf2 * f2;
  }
}

// NP = 1 or 2 pose sets.  NP = 2 (the paired launch) reads the operand stream ONCE and accumulates the moments of two sets of relative transforms (rel, x.rel2)
// side by side: same loads, same chunk order, every expression of a set exactly the one-pose build's, each set reduced through LDS in the same fixed order ->
// partials bit-identical to two one-pose launches.  The second set's partials follow the first's at x.partials2_off doubles.  2 x 28 / 29 fp64 accumulators
// per lane: 2 waves per SIMD instead of 3, no spills.
template <bool PLANE, bool ROBUST, int NP>
__global__ __launch_bounds__(NT) void linearize_kernel(const int* __restrict__ chunk_edge, const int* __restrict__ chunk_start, int chunk,
                                                       const int* __restrict__ count, const long long* __restrict__ cap_off, long long total_cap,
                                                       const double* __restrict__ rel, const double* __restrict__ a_scale,
                                                       const double* __restrict__ stream, double* __restrict__ partials,
                                                       const double* const* __restrict__ src_pts, const int* __restrict__ nsrc,
                                                       const int* __restrict__ chunk_first, PairArgs<NP> x) {
  const int e = chunk_edge[blockIdx.x];
  const int start = chunk_start[blockIdx.x];
  // the partial's slot is the chunk's place in ITS EDGE's run (chunk_first[e] + k), whatever the launch order of the workgroups (api.cpp interleaves the chunks
  // of the edges that share a source cloud, so that the second reader of a piece of p finds it in the same XCD's L2); reduce_expand_kernel sums an edge's slots
  // in order, so the result does not depend on that order
  const int c = chunk_first[e] + start / chunk;
  const int cnt = count[e];
  if (start >= cnt) return;
  const int end = min(cnt, start + chunk);
  __shared__ double srel[NP][kEdgeRel];
  __shared__ double red[NACC / 2][NT + 1];
  if (threadIdx.x < kEdgeRel) srel[0][threadIdx.x] = rel[(size_t)e * kEdgeRel + threadIdx.x];
  if constexpr (NP > 1) { if (threadIdx.x >= 32 && threadIdx.x < 32 + kEdgeRel) srel[1][threadIdx.x - 32] = x.rel2[(size_t)e * kEdgeRel + threadIdx.x - 32]; }
  __syncthreads();
  double A[NP][9], t[NP][3];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int i = 0; i < 9; ++i) A[k][i] = srel[k][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[k][i] = srel[k][9 + i];
  }
  double inv_a2 = 1.0;
  if (ROBUST) { const double a = a_scale[e]; inv_a2 = 1.0 / (a * a); }

  double acc[NP][NACC];
#pragma unroll
  for (int k = 0; k < NP; ++k)
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[k][i] = 0.0;

  const size_t base = (size_t)cap_off[e];  // multiple of 64 -> 16-B aligned double2 loads
  const double* __restrict__ s0 = stream + base;
  constexpr int NS = PLANE ? 7 : 6;
  // register slot j -> stream array: plane p n c = arrays 0..6; point p q = arrays 0-2, 7-9
  auto arr = [](int j) { return PLANE ? j : (j < 3 ? j : j + 4); };
  // two adjacent correspondences per lane per step (16-B loads); the next step's loads are issued before
  // the current step's arithmetic so two steps of HBM latency overlap.
  int pos = start + 2 * threadIdx.x;
  double2 cur[9], nxt[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) { cur[j] = make_double2(0.0, 0.0); nxt[j] = make_double2(0.0, 0.0); }
  // Every query accepted (count == N_src: the usual case once the clouds overlap within the cutoff) makes the list the identity,
  // first[pos] = pos, so p is the source cloud itself in its sorted order: read it from there (AoS, three 16-B loads per pair of
  // correspondences, ordinary cacheable loads) instead of from the stream's private copy.  The two edges of a source frame are
  // consecutive in the chunk order and share that 24 B per point through L2 / MALL — same values, so results are bit-identical.
  const double* __restrict__ sp = (src_pts != nullptr && cnt == nsrc[e]) ? src_pts[e] : nullptr;
  auto load = [&](double2 (&v)[9], int at) {
    if (at + 1 < end) {
      if (sp != nullptr) {
        const double2 a = *reinterpret_cast<const double2*>(sp + 3 * (size_t)at);
        const double2 b = *reinterpret_cast<const double2*>(sp + 3 * (size_t)at + 2);
        const double2 c2 = *reinterpret_cast<const double2*>(sp + 3 * (size_t)at + 4);
        v[0] = make_double2(a.x, b.y); v[1] = make_double2(a.y, c2.x); v[2] = make_double2(b.x, c2.y);
      }
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        if (j < 3 && sp != nullptr) continue;
        // non-temporal: the stream is read exactly once per evaluation and is larger than the caches; keeping it from
        // allocating there is worth +15 % bandwidth (cfg4 136 -> 117 us, cfg5 6.3 -> 7.0 TB/s)
        typedef double d2v __attribute__((ext_vector_type(2)));
        const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(s0 + (size_t)arr(j) * total_cap + at));
        v[j] = make_double2(t.x, t.y);
      }
    } else if (at < end) {
#pragma unroll
      for (int j = 0; j < NS; ++j) { v[j].x = (j < 3 && sp != nullptr) ? sp[3 * (size_t)at + j] : s0[(size_t)arr(j) * total_cap + at]; v[j].y = 0.0; }
    }
  };
  load(cur, pos);
  while (pos < end) {
    const int npos = pos + 2 * NT;
    load(nxt, npos);
    // slots: plane 0-2 p, 3-5 n, 6 c;  point 0-2 p, 3-5 q
    // (pose set k of NP; spelled out rather than looped: a loop here, even of one trip, changes the schedule of the one-pose build)
#define MVICP_LIN_STEP(k)                                                                                                                                   \
    if (PLANE) {                                                                                                                                            \
      accumulate<PLANE, ROBUST>(acc[k], A[k], t[k], inv_a2, cur[0].x, cur[1].x, cur[2].x, cur[6].x, 0.0, 0.0, cur[3].x, cur[4].x, cur[5].x);             \
      if (pos + 1 < end)                                                                                                                                    \
        accumulate<PLANE, ROBUST>(acc[k], A[k], t[k], inv_a2, cur[0].y, cur[1].y, cur[2].y, cur[6].y, 0.0, 0.0, cur[3].y, cur[4].y, cur[5].y);           \
    } else {                                                                                                                                                \
      accumulate<PLANE, ROBUST>(acc[k], A[k], t[k], inv_a2, cur[0].x, cur[1].x, cur[2].x, cur[3].x, cur[4].x, cur[5].x, 0.0, 0.0, 0.0);                  \
      if (pos + 1 < end)                                                                                                                                    \
        accumulate<PLANE, ROBUST>(acc[k], A[k], t[k], inv_a2, cur[0].y, cur[1].y, cur[2].y, cur[3].y, cur[4].y, cur[5].y, 0.0, 0.0, 0.0);                \
    }
    MVICP_LIN_STEP(0)
    if constexpr (NP > 1) { MVICP_LIN_STEP(NP - 1) }
#undef MVICP_LIN_STEP
#pragma unroll
    for (int j = 0; j < 9; ++j) cur[j] = nxt[j];
    pos = npos;
  }

  // each pose set through the one block reduction (lin_common.h), the second after a barrier on the rows the first still reads
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    double* __restrict__ pk = partials;
    if constexpr (NP > 1) { if (k) pk = partials + x.partials2_off; }
    block_reduce_store(acc[k], red, pk, c, k != 0);
  }
}

}  // namespace

// algorithmic bytes of one pass over the operand stream: 32 B (plane: n, n.q) / 24 B (point: q) per correspondence + the source point p, 24 B — per correspondence
// when the edge reads its private copy from the stream, ONCE PER SOURCE POINT for the edges of one source cloud that read the shared sorted cloud side by side
// (identity lists, lin_share_p + lin_interleave: the second edge's read is an L2 hit by construction; PMC: 0.695 -> 0.551 GB per launch at cfg4)
static double stream_pass_bytes(mvicp_ctx* c, int plane) {
  double bytes = 0;
  std::vector<char> src_counted((size_t)c->n_frames, 0);
  for (int e = 0; e < c->E; ++e) {
    if (!c->owned[e]) continue;
    const double cnt = c->hist.h_count[e];
    const int s = c->esrc[e];
    bytes += (plane ? 32.0 : 24.0) * cnt;
    if (c->lin_share_p && c->lin_interleave && c->hist.h_count[e] == c->frames[s].n) { if (!src_counted[s]) { bytes += 24.0 * cnt; src_counted[s] = 1; } }
    else bytes += 24.0 * cnt;
  }
  return bytes;
}

int launch_linearize(mvicp_ctx* c, int plane, int robust) {
  if (c->E == 0) return MVICP_OK;
  const int chunk = c->lin_chunk;
  if (c->n_chunks > 0) {
    const double bytes = stream_pass_bytes(c, plane);
    const double* const* d_src = nullptr;
    MV_CHECK(source_table(c, &d_src));
    ProfScope ps(c, "linearize", bytes);
#define LAUNCH(P, R)                                                                                                                           \
  hipLaunchKernelGGL((linearize_kernel<P, R, 1>), dim3(c->n_lin_wg), dim3(NT), 0, c->stream, c->d_chunk_edge, c->d_chunk_start, chunk, c->d_count, \
                     c->d_cap_off, c->total_cap, c->d_rel, c->d_a, c->d_stream, c->d_partials, d_src, (const int*)c->d_nsrc, (const int*)c->d_chunk_first, PairArgs<1>{})
    if (plane && robust) LAUNCH(true, true);
    else if (plane) LAUNCH(true, false);
    else if (robust) LAUNCH(false, true);
    else LAUNCH(false, false);
#undef LAUNCH
  }
  {
    ProfScope ps(c, "reduce", 0.0);
    if (plane)
      hipLaunchKernelGGL((reduce_expand_kernel<true, 1>), dim3(c->E), dim3(256), 0, c->stream, c->d_chunk_first, chunk, c->d_count, c->d_rel, c->d_partials, c->lin_out ? c->lin_out : c->d_out, PairArgs<1>{});
    else
      hipLaunchKernelGGL((reduce_expand_kernel<false, 1>), dim3(c->E), dim3(256), 0, c->stream, c->d_chunk_first, chunk, c->d_count, c->d_rel, c->d_partials, c->lin_out ? c->lin_out : c->d_out, PairArgs<1>{});
  }
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

// Two evaluations on the same correspondences and scales in ONE pass over the stream: the blocks at the relative transforms in d_rel go to out_a, those at
// d_rel2 to out_b — what launch_linearize would give for each, bit for bit.  The profile scope is its own ("linearize_pair", bytes of one pass).
int launch_linearize_pair(mvicp_ctx* c, int plane, int robust, double* out_a, double* out_b) {
  if (c->E == 0) return MVICP_OK;
  const int chunk = c->lin_chunk;
  PairArgs<2> x;
  x.rel2 = c->d_rel2; x.partials2_off = (size_t)c->n_chunks * kLinPartial; x.out2 = out_b;
  if (c->n_chunks > 0) {
    const double bytes = stream_pass_bytes(c, plane);
    const double* const* d_src = nullptr;
    MV_CHECK(source_table(c, &d_src));
    ProfScope ps(c, "linearize_pair", bytes);
#define LAUNCH(P, R)                                                                                                                              \
  hipLaunchKernelGGL((linearize_kernel<P, R, 2>), dim3(c->n_lin_wg), dim3(NT), 0, c->stream, c->d_chunk_edge, c->d_chunk_start, chunk, c->d_count, \
                     c->d_cap_off, c->total_cap, c->d_rel, c->d_a, c->d_stream, c->d_partials, d_src, (const int*)c->d_nsrc, (const int*)c->d_chunk_first, x)
    if (plane && robust) LAUNCH(true, true);
    else if (plane) LAUNCH(true, false);
    else if (robust) LAUNCH(false, true);
    else LAUNCH(false, false);
#undef LAUNCH
  }
  {
    ProfScope ps(c, "reduce", 0.0);
    if (plane)
      hipLaunchKernelGGL((reduce_expand_kernel<true, 2>), dim3(c->E, 2), dim3(256), 0, c->stream, c->d_chunk_first, chunk, c->d_count, c->d_rel, c->d_partials, out_a, x);
    else
      hipLaunchKernelGGL((reduce_expand_kernel<false, 2>), dim3(c->E, 2), dim3(256), 0, c->stream, c->d_chunk_first, chunk, c->d_count, c->d_rel, c->d_partials, out_a, x);
  }
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

}  // namespace mvicp
