// The per-point part of the jet fit that normals_jet.hip (mvicp_fit_normals) and smooth.hip (mvicp_smooth_points) share: the tangent frame,
// the normal equations by shared tree sums and the Cholesky factorisation with the forward solve carried along.  One wave per point, lane t = entry t of the row.  The contract is stated in include/mvicp.h.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
#pragma once
#include "common.h"

namespace mvicp {
namespace jet {

constexpr int kWavesPerBlock = 4;

__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
constexpr int pow2_ceil(int n) { int b = 1; while (b < n) b <<= 1; return b; }

// One step of the tree for W sums at once, across the lane bit X: of each pair (y[2i], y[2i+1]) a lane keeps the one its bit X selects, sends
// the other to its partner and adds what it receives -- y[u] <- y[2u] + y[2u+1] of the contract's tree for both sums, IEEE addition being
// commutative, with one shuffle where two butterflies take two.  W / 2 sums remain per lane.
template <int W, int X> __device__ __forceinline__ void scatter_step(double* y, int lane) {
  if constexpr (W > 1) {
    const bool up = (lane & X) != 0;
#pragma unroll
    for (int i = 0; i < W / 2; ++i) {
      const double keep = up ? y[2 * i + 1] : y[2 * i], send = up ? y[2 * i] : y[2 * i + 1];
      y[i] = __dadd_rn(keep, __shfl_xor(send, X, 64));
    }
    scatter_step<W / 2, 2 * X>(y, lane);
  }
}
// T of B sums (a power of two, <= 64) whose lane values are y[0 .. B-1]: lane l ends with T of sum l & (B - 1).  The first log2(B) levels of the
// tree are scatter steps, the rest the plain butterfly on the one value left.  y is used up.
template <int B> __device__ __forceinline__ double scatter_tree_sum(double (&y)[B], int lane) {
  scatter_step<B, 1>(y, lane);
  double v = y[0];
#pragma unroll
  for (int x = B; x < 64; x <<= 1) v = __dadd_rn(v, __shfl_xor(v, x, 64));
  return v;
}
// lane `src`'s value (src a constant) in every lane
__device__ __forceinline__ double lane_value(double v, int src) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// the largest of the 64 lanes' values (none is a NaN, none negative), in every lane
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) { const double o = __shfl_xor(v, x, 64); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ bool finite(double v) { return fabs(v) < __builtin_huge_val(); }

// Column J of the Cholesky factorisation L (L[r][c], r >= c) with the forward solve y carried along as one more row.  The column's sums --
// G_JJ, G_rJ for r > J and r_J -- are formed here, together, by one scatter_tree_sum; lane e then holds the e-th of them.
template <int M, int J> __device__ __forceinline__ void jet_column(const double (&b)[M], double Z, int lane, double (&L)[M][M], double (&y)[M], bool& ok) {
  constexpr int N = M - J + 1, B = pow2_ceil(N);
  double t[B];
#pragma unroll
  for (int r = J; r < M; ++r) t[r - J] = __dmul_rn(b[J], b[r]);
  t[M - J] = __dmul_rn(b[J], Z);
#pragma unroll
  for (int e = N; e < B; ++e) t[e] = 0.0;
  const double sums = scatter_tree_sum<B>(t, lane);
  const double Gjj = lane_value(sums, 0);
  double s = Gjj;
#pragma unroll
  for (int q = 0; q < J; ++q) s = __dsub_rn(s, __dmul_rn(L[J][q], L[J][q]));
  ok = ok && s > __dmul_rn(0x1p-20, Gjj);
  const double Ljj = __dsqrt_rn(s);
  L[J][J] = Ljj;
#pragma unroll
  for (int r = J + 1; r < M; ++r) {
    s = lane_value(sums, r - J);
#pragma unroll
    for (int q = 0; q < J; ++q) s = __dsub_rn(s, __dmul_rn(L[r][q], L[J][q]));
    L[r][J] = __ddiv_rn(s, Ljj);
  }
  s = lane_value(sums, M - J);
#pragma unroll
  for (int q = 0; q < J; ++q) s = __dsub_rn(s, __dmul_rn(L[J][q], y[q]));
  y[J] = __ddiv_rn(s, Ljj);
  if constexpr (J + 1 < M) jet_column<M, J + 1>(b, Z, lane, L, y, ok);
}

// The tangent frame from n alone (step 4): w = e_a x n for the axis a of the smallest |n_a|, the first of equals; u = w / |w|, v = n x u.
struct Tangent { double u0, u1, u2, v0, v1, v2; };
__device__ __forceinline__ Tangent tangent_frame(double nx, double ny, double nz) {
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  const bool s1 = ay < ax;
  const bool s2 = az < (s1 ? ay : ax);
  const double w0 = s2 ? -ny : s1 ? nz : 0.0, w1 = s2 ? nx : s1 ? 0.0 : -nz, w2 = s2 ? 0.0 : s1 ? -nx : ny;
  const double lw = __dsqrt_rn(dot3(w0, w1, w2, w0, w1, w2));
  Tangent f;
  f.u0 = __ddiv_rn(w0, lw); f.u1 = __ddiv_rn(w1, lw); f.u2 = __ddiv_rn(w2, lw);
  f.v0 = __dsub_rn(__dmul_rn(ny, f.u2), __dmul_rn(nz, f.u1)); f.v1 = __dsub_rn(__dmul_rn(nz, f.u0), __dmul_rn(nx, f.u2));
  f.v2 = __dsub_rn(__dmul_rn(nx, f.u1), __dmul_rn(ny, f.u0));
  return f;
}

}  // namespace jet
}  // namespace mvicp
