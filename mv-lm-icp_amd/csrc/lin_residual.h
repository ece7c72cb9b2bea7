// The compensated residual f = A p + t - q that the symmetric (linearize_sym.hip) and the plane-to-plane (linearize_gicp.hip) kernels share.
#pragma once

namespace mvicp {

namespace {

// s = fl(a + b) and e with a + b = s + e exactly (Knuth's TwoSum: no assumption on the magnitudes)
__device__ __forceinline__ double two_sum(double a, double b, double& e) {
#pragma clang fp contract(off)
  const double s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
  return s;
}

// One component of f = A p + t - q, a small difference of large terms, to a relative error of a few 2^-53 OF f ITSELF: the three products with their exact
// errors (fma), the five terms added by TwoSum, the errors and the low parts of (A, t) added at the end.  The plain form ((x' + t) - q) carries the rounding of
// x' and of x' + t, 2^-53 (|x'| + |t|) per correspondence: against residuals of 5e-4 on clouds of extent 0.4 that is 1e-14 of the cost and of g over 1 500
// correspondences — the size of a plain fp64 evaluation's own error there, and over 32 x it whenever that evaluation happens to be lucky
// (tests/test_gpu_sym_regimes.py met that in 6 of 4 140 pieces).  The 37 flops per component are NOT hidden behind the operand traffic at two waves per SIMD:
// measured at cfg4's shape the launch went from 153 to 166 - 173 us.
// Contraction is switched off in both functions: a product fused into the sum that follows it would make that sum something other than fl(h_0 + h_1).
__device__ __forceinline__ double residual_component(double a0, double a1, double a2, double t, double p0, double p1, double p2, double q, double lo) {
#pragma clang fp contract(off)
  const double h0 = a0 * p0, h1 = a1 * p1, h2 = a2 * p2;
  const double g0 = __builtin_fma(a0, p0, -h0), g1 = __builtin_fma(a1, p1, -h1), g2 = __builtin_fma(a2, p2, -h2);
  double e1, e2, e3, e4;
  const double s1 = two_sum(h0, h1, e1);
  const double s2 = two_sum(s1, h2, e2);
  const double s3 = two_sum(s2, t, e3);
  const double s4 = two_sum(s3, -q, e4);
  return s4 + ((((e1 + e2) + (e3 + e4)) + ((g0 + g1) + g2)) + lo);
}

}  // namespace

}  // namespace mvicp
