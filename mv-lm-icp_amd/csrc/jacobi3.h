// The 3 x 3 cyclic Jacobi rotation that every eigen-solve of the library uses (normals_pca.h: the PCA normal of mvicp_estimate_normals;
// iss.hip: the keypoint eigenvalues; normals.hip: the reference-parity normal).  Every fp64 operation is an __d*_rn intrinsic: rounded
// on its own, never contracted into an fma.  How many sweeps run, and any exit test between them, is the caller's.
#pragma once
#include <hip/hip_runtime.h>

namespace mvicp {
namespace jacobi3 {

// a 3 x 3 matrix in nine named registers: every index below is a template argument, so nothing is addressed at run time
struct M33 { double m00, m01, m02, m10, m11, m12, m20, m21, m22; };
template <int R, int C> __device__ __forceinline__ double& at(M33& m) {
  if constexpr (R == 0) { if constexpr (C == 0) return m.m00; else if constexpr (C == 1) return m.m01; else return m.m02; }
  else if constexpr (R == 1) { if constexpr (C == 0) return m.m10; else if constexpr (C == 1) return m.m11; else return m.m12; }
  else { if constexpr (C == 0) return m.m20; else if constexpr (C == 1) return m.m21; else return m.m22; }
}
// columns P, Q: (x[r][P], x[r][Q]) <- (c x[r][P] - s x[r][Q], s x[r][P] + c x[r][Q])
template <int R, int P, int Q> __device__ __forceinline__ void rot_cols(M33& x, double c, double s) {
  const double xp = at<R, P>(x), xq = at<R, Q>(x);
  at<R, P>(x) = __dsub_rn(__dmul_rn(c, xp), __dmul_rn(s, xq)); at<R, Q>(x) = __dadd_rn(__dmul_rn(s, xp), __dmul_rn(c, xq));
}
template <int R, int P, int Q> __device__ __forceinline__ void rot_rows(M33& x, double c, double s) {
  const double xp = at<P, R>(x), xq = at<Q, R>(x);
  at<P, R>(x) = __dsub_rn(__dmul_rn(c, xp), __dmul_rn(s, xq)); at<Q, R>(x) = __dadd_rn(__dmul_rn(s, xp), __dmul_rn(c, xq));
}
// one rotation on the pair (P, Q), P < Q: it annihilates A[P][Q], read from the upper triangle.  VEC: V <- V J as well (V unused otherwise)
template <int P, int Q, bool VEC> __device__ __forceinline__ void rotate(M33& A, M33& V) {
  const double apq = at<P, Q>(A);
  if (apq == 0.0) return;
  const double theta = __ddiv_rn(__dsub_rn(at<Q, Q>(A), at<P, P>(A)), __dmul_rn(2.0, apq));
  const double t = __ddiv_rn(theta >= 0 ? 1.0 : -1.0, __dadd_rn(fabs(theta), __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0))));
  const double c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0))), s = __dmul_rn(t, c);
  rot_cols<0, P, Q>(A, c, s); rot_cols<1, P, Q>(A, c, s); rot_cols<2, P, Q>(A, c, s);   // A <- A J
  rot_rows<0, P, Q>(A, c, s); rot_rows<1, P, Q>(A, c, s); rot_rows<2, P, Q>(A, c, s);   // A <- J^T A
  if constexpr (VEC) { rot_cols<0, P, Q>(V, c, s); rot_cols<1, P, Q>(V, c, s); rot_cols<2, P, Q>(V, c, s); }   // V <- V J
}
// one sweep over (0,1), (0,2), (1,2): with the vectors, and the diagonal alone
__device__ __forceinline__ void sweep(M33& A, M33& V) { rotate<0, 1, true>(A, V); rotate<0, 2, true>(A, V); rotate<1, 2, true>(A, V); }
__device__ __forceinline__ void sweep(M33& A) { rotate<0, 1, false>(A, A); rotate<0, 2, false>(A, A); rotate<1, 2, false>(A, A); }

}  // namespace jacobi3
}  // namespace mvicp
