// What the translation units of the linearization share (linearize.hip: point-to-point and point-to-plane; linearize_sym.hip: the symmetric
// objective; linearize_gicp.hip: plane-to-plane): the launch constants, the robust-loss helpers, the extra arguments of a paired launch, the block
// reduction that ends every accumulation kernel (block_reduce_store), and the per-edge reduce + expansion
// kernel, which every family runs behind its own accumulation kernel, and the host table of the per-edge sorted source clouds.  The rest of what the two
// normal-carrying families share — the body of their kernels and their host launch — is in lin_normal.h.  Everything sits in an anonymous namespace, as it did inside
// linearize.hip: each unit gets its own internal copy, under the same names.
#pragma once
#include "common.h"

namespace mvicp {

namespace {

constexpr int NT = kLinThreads;
constexpr int NB = MVICP_EDGE_BLOCK;  // 91
constexpr int NACC = kLinPartial;     // padded partial width (28 plane / 29 point)

// rho / 2 = a^2 (sqrt(y) - 1) with y = 1 + s / a^2, written as s w / (1 + w) with w = 1 / sqrt(y): the textbook form cancels for a >> |r| (y -> 1: every term
// is rounded to an ulp of 1, 1e-4 relative at a = 1e6 |r|), this one is good to a few ulp of the term at every a and is exactly 0 for s = 0.
// 1 / (1 + w), 1 + w in (1, 2]: v_rcp_f64 seed + two Newton steps.
__device__ __forceinline__ double half_rho(double s, double w) {
  const double d = 1.0 + w;
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  return (s * w) * r;
}

__device__ __forceinline__ double fast_rsqrt(double y) {
  // y in [1, huge): v_rsq_f64 seed + two Newton steps (each squares the error) -> ~1 ulp
  double r = __builtin_amdgcn_rsq(y);
  r = r * (1.5 - 0.5 * y * r * r);
  r = r * (1.5 - 0.5 * y * r * r);
  return r;
}

// Extra kernel arguments of the two-pose builds (empty for one pose set, so the one-pose kernels keep their argument layout).
template <int NP> struct PairArgs {};
template <> struct PairArgs<2> { const double* rel2; size_t partials2_off; double* out2; };

// Block reduction of one workgroup's NACC sums through LDS, transposed, into partial slot c of pk: every thread stores value j into row j (stride-1
// across lanes: conflict-free ds_write_b64), then 16 threads per row add 16 columns each and finish with a 4-step xor-shuffle inside their lane group
// (two passes of 16 rows keep the LDS footprint at 33 KB).  Fixed association order -> deterministic, and the same for every family.
// lead_sync: red is still being read (a second reduction through the same rows), so a barrier comes first.
__device__ __forceinline__ void block_reduce_store(const double (&acc)[NACC], double (&red)[NACC / 2][NT + 1], double* __restrict__ pk, int c, bool lead_sync) {
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass || lead_sync) __syncthreads();
#pragma unroll
    for (int j = 0; j < NACC / 2; ++j) red[j][threadIdx.x] = acc[pass * (NACC / 2) + j];
    __syncthreads();
    const int row = threadIdx.x >> 4, part = threadIdx.x & 15;  // 16 rows x 16 parts
    double sum = 0.0;
#pragma unroll 8
    for (int i = 0; i < NT / 16; ++i) sum += red[row][part + 16 * i];
    sum += __shfl_xor(sum, 1, 64);
    sum += __shfl_xor(sum, 2, 64);
    sum += __shfl_xor(sum, 4, 64);
    sum += __shfl_xor(sum, 8, 64);
    if (part == 0) pk[(size_t)c * NACC + pass * (NACC / 2) + row] = sum;
  }
}

// ---- per edge: fixed-order sum of the workgroup partials, then expansion to the canonical 12x12 block
__device__ __forceinline__ void cross_mat(const double* a, double* M) {  // row-major [a]x
  M[0] = 0; M[1] = -a[2]; M[2] = a[1];
  M[3] = a[2]; M[4] = 0; M[5] = -a[0];
  M[6] = -a[1]; M[7] = a[0]; M[8] = 0;
}

// NP = 2: blockIdx.y picks the pose set of a paired launch (its relative transforms, partials and output); per set the same arithmetic
template <bool PLANE, int NP>
__global__ __launch_bounds__(256) void reduce_expand_kernel(const int* __restrict__ chunk_first, int chunk, const int* __restrict__ count,
                                                           const double* __restrict__ rel, const double* __restrict__ partials,
                                                           double* __restrict__ out, PairArgs<NP> x) {
  if constexpr (NP > 1) {
    if (blockIdx.y) { rel = x.rel2; partials += x.partials2_off; out = x.out2; }
  }
  const int e = blockIdx.x;
  const int tid = threadIdx.x;
  __shared__ double m[8][NACC];
  __shared__ double S[36], X[36], Y[36], R6[36], Lm[36], T1[36], T2[36], T3[36], H[144], v[6];
  const int c0 = chunk_first[e];
  const int nchunks = min(chunk_first[e + 1] - c0, (count[e] + chunk - 1) / chunk);
  {
    // 256 threads: eight interleaved fixed-order partial sums per value (short dependent-load chains), combined in fixed order
    const int val = tid & (NACC - 1), part = tid >> 5;
    double s = 0.0;
    for (int c = part; c < nchunks; c += 8) s += partials[(size_t)(c0 + c) * NACC + val];
    m[part][val] = s;
  }
  if (tid < 36) { S[tid] = 0.0; X[tid] = 0.0; Y[tid] = 0.0; R6[tid] = 0.0; Lm[tid] = (tid / 6 == tid % 6) ? 1.0 : 0.0; }
  __syncthreads();
  if (tid < NACC) {
    double s = m[0][tid];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += m[k][tid];
    m[0][tid] = s;
  }
  __syncthreads();
  const double* mm = m[0];
  const double* A = rel + (size_t)e * kEdgeRel;  // column-major 3x3
  const double* t = A + 9;
  if (tid < 9) {
    // R6 = diag(A, A),  L = [[I, 0],[[t]x, I]]   (row-major 6x6)
    const int i = tid / 3, j = tid % 3;
    double tx[9];
    cross_mat(t, tx);
    const double a = A[i + 3 * j];
    R6[i * 6 + j] = a;
    R6[(3 + i) * 6 + 3 + j] = a;
    Lm[(3 + i) * 6 + j] = tx[i * 3 + j];
    if (PLANE) {
      if (tid < 6) v[tid] = mm[21 + tid];
    } else {
      const double w = mm[0];
      const double px[3] = {mm[1], mm[2], mm[3]};
      const double P[9] = {mm[4], mm[5], mm[6], mm[5], mm[7], mm[8], mm[6], mm[8], mm[9]};            // sum w x' x'^T
      const double rr[3] = {mm[10], mm[11], mm[12]};
      const double PR[9] = {mm[13], mm[14], mm[15], mm[16], mm[17], mm[18], mm[19], mm[20], mm[21]};  // sum w x' r^T (row-major)
      const double RR[9] = {mm[22], mm[23], mm[24], mm[23], mm[25], mm[26], mm[24], mm[26], mm[27]};
      double pxm[9], rxm[9];
      cross_mat(px, pxm);
      cross_mat(rr, rxm);
      const double trP = P[0] + P[4] + P[8], trRR = RR[0] + RR[4] + RR[8], trPR = PR[0] + PR[4] + PR[8];
      const double I = i == j ? 1.0 : 0.0;
      // (x' = A p throughout)  S = sum w [[I, -[x']x],[[x']x, |x'|^2 I - x' x'^T]]
      S[i * 6 + j] = w * I;
      S[i * 6 + 3 + j] = -pxm[i * 3 + j];
      S[(3 + i) * 6 + j] = pxm[i * 3 + j];
      S[(3 + i) * 6 + 3 + j] = trP * I - P[i * 3 + j];
      // X = sum w [[0, -[r]x],[0, -[x']x[r]x]],  [x']x[r]x = r x'^T - (x'.r) I
      X[i * 6 + 3 + j] = -rxm[i * 3 + j];
      X[(3 + i) * 6 + 3 + j] = -(PR[j * 3 + i] - trPR * I);
      // Y = sum w [[0,0],[0, |r|^2 I - r r^T]]
      Y[(3 + i) * 6 + 3 + j] = trRR * I - RR[i * 3 + j];
      if (tid == 0) {
        // v = sum w [r ; x' x r],  (x' x r) from the antisymmetric part of x' r^T
        v[0] = rr[0]; v[1] = rr[1]; v[2] = rr[2];
        v[3] = PR[1 * 3 + 2] - PR[2 * 3 + 1];
        v[4] = PR[2 * 3 + 0] - PR[0 * 3 + 2];
        v[5] = PR[0 * 3 + 1] - PR[1 * 3 + 0];
      }
    }
  }
  if (PLANE && tid >= 16 && tid < 16 + 21) {
    // unpack U (upper triangle, row-major) into the full symmetric S
    const int k = tid - 16;
    int i = 0, o = k;
    while (o >= 6 - i) { o -= 6 - i; ++i; }
    const int j = i + o;
    S[i * 6 + j] = mm[k];
    S[j * 6 + i] = mm[k];
  }
  __syncthreads();
  if (tid < 36) {
    const int i = tid / 6, j = tid % 6;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += S[i * 6 + k] * R6[k * 6 + j];
    T1[tid] = s;                                                    // S R6
    T2[tid] = S[tid] - X[tid];                                      // Z = S - X
    T3[tid] = S[tid] - X[tid] - X[j * 6 + i] + Y[tid];              // D = S - X - X^T + Y
  }
  __syncthreads();
  double zl = 0.0, dl = 0.0;
  if (tid < 36) {
    const int i = tid / 6, j = tid % 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) { zl += T2[i * 6 + k] * Lm[j * 6 + k]; dl += T3[i * 6 + k] * Lm[j * 6 + k]; }
  }
  __syncthreads();
  if (tid < 36) { T2[tid] = zl; T3[tid] = dl; }                     // Z L^T, D L^T
  __syncthreads();
  double* o = out + (size_t)e * NB;
  if (tid < 36) {
    const int i = tid / 6, j = tid % 6;
    double hss = 0.0, hsd = 0.0, hdd = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { hss += R6[k * 6 + i] * T1[k * 6 + j]; hsd += R6[k * 6 + i] * T2[k * 6 + j]; hdd += Lm[i * 6 + k] * T3[k * 6 + j]; }
    H[i * 12 + j] = hss;                       // H_ss = R6^T S R6
    H[i * 12 + 6 + j] = -hsd;                  // H_sd = -R6^T (S - X) L^T
    H[(6 + i) * 12 + 6 + j] = hdd;             // H_dd = L (S - X - X^T + Y) L^T
  } else if (tid < 42) {
    const int i = tid - 36;
    double s = 0.0, l = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) { s += R6[k * 6 + i] * v[k]; l += Lm[i * 6 + k] * v[k]; }
    o[78 + i] = s;           // g_s = R6^T v
    o[84 + i] = -l;          // g_d = -L v
  } else if (tid == 42) {
    o[90] = count[e] > 0 ? mm[PLANE ? 27 : 28] : 0.0;
  }
  __syncthreads();
  for (int k = tid; k < 78; k += 256) {
    int i = 0, r = k;
    while (r >= 12 - i) { r -= 12 - i; ++i; }
    const int j = i + r;
    // H_ss and H_dd are symmetric up to rounding: average the two triangles so the block is exactly symmetric
    o[k] = (i < 6 && j >= 6) ? H[i * 12 + j] : 0.5 * (H[i * 12 + j] + H[j * 12 + i]);
  }
}

// per-edge sorted source clouds (identity-list fast path of the kernel); table cached by content
static int source_table(mvicp_ctx* c, const double* const** d_src) {
  *d_src = nullptr;
  if (c->lin_share_p) {
    std::vector<const double*> tab((size_t)c->E, nullptr);
    for (int e = 0; e < c->E; ++e) if (c->owned[e]) tab[e] = c->frames[c->esrc[e]].grid.spts;
    MV_CHECK(cached_upload(c, "lin_src", tab.data(), sizeof(void*) * tab.size(), (void**)d_src));
  }
  return MVICP_OK;
}

// algorithmic bytes of one symmetric or plane-to-plane pass (linearize_sym.hip, linearize_gicp.hip: the same operands by the same routes):
// 48 B (n_q, q) per correspondence + 24 B p + 24 B n_p — per correspondence, plus the 4-B index, when the edge
// reads its private p from the stream and gathers n_p, ONCE PER SOURCE POINT for the edges of one source cloud that read the sorted cloud side by side.
// The condition is the kernel's own: a searched list that holds every source point with lin_share_p on (an explicit list never is the identity,
// mvicp_set_correspondences), and the second reader's hit needs lin_interleave; stream_pass_bytes in linearize.hip is coarser on both points.
static double sym_pass_bytes(mvicp_ctx* c) {
  double bytes = 0;
  std::vector<char> src_counted((size_t)c->n_frames, 0);
  for (int e = 0; e < c->E; ++e) {
    if (!c->owned[e]) continue;
    const double cnt = c->hist.h_count[e];
    const int s = c->esrc[e];
    bytes += 48.0 * cnt;
    if (c->lin_share_p && !c->hist.explicit_list[e] && c->hist.h_count[e] == c->frames[s].n) {
      if (!c->lin_interleave) bytes += 48.0 * cnt;
      else if (!src_counted[s]) { bytes += 48.0 * cnt; src_counted[s] = 1; }
    } else {
      bytes += 52.0 * cnt;
    }
  }
  return bytes;
}

}  // namespace

}  // namespace mvicp
