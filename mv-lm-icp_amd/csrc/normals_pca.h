// The per-point part of mvicp_estimate_normals that normals_pca.hip and normals_jet.hip share: the gather of a row's offsets, the tree sum,
// the 3 x 3 Jacobi iteration (jacobi3.h) and the oriented PCA normal with its surface variation.  One wave per point, lane t = entry t of the row.
// Every fp64 operation is an __d*_rn intrinsic: rounded on its own, never contracted into an fma.
#pragma once
#include "common.h"
#include "jacobi3.h"

namespace mvicp {
namespace pca {

constexpr int kSweeps = 6;
using jacobi3::M33;

// T(y): the sum of the 64 lanes' values in the order of the contract's tree, in every lane
__device__ __forceinline__ double tree_sum(double v) {
#pragma unroll
  for (int x = 1; x < 64; x <<= 1) v = __dadd_rn(v, __shfl_xor(v, x, 64));
  return v;
}

// lane t's offset d = p_j - p_i for entry t of row i (k entries wide, len of them filled); lanes past the row carry +0.0
__device__ __forceinline__ void row_offset(const double* __restrict__ pts, const int* __restrict__ idx, int i, int k, int len, int lane, double px, double py,
                                           double pz, double& d0, double& d1, double& d2) {
  d0 = 0.0; d1 = 0.0; d2 = 0.0;
  if (lane < len) {
    const double* pj = pts + 3 * (size_t)idx[(size_t)i * (size_t)k + lane];
    d0 = __dsub_rn(pj[0], px); d1 = __dsub_rn(pj[1], py); d2 = __dsub_rn(pj[2], pz);
  }
}

// the contract's normal (nx, ny, nz) and curvature cv of the point (px, py, pz) from the wave's offsets, in every lane; len < 3: zeros
__device__ __forceinline__ void point_normal(double d0, double d1, double d2, int len, int lane, double px, double py, double pz, double vx, double vy,
                                             double vz, double& nx, double& ny, double& nz, double& cv) {
  nx = 0.0; ny = 0.0; nz = 0.0; cv = 0.0;
  if (len >= 3) {   // (wave-uniform)
    const double c = (double)len;
    const double m0 = __ddiv_rn(tree_sum(d0), c), m1 = __ddiv_rn(tree_sum(d1), c), m2 = __ddiv_rn(tree_sum(d2), c);
    const bool in = lane < len;
    const double x0 = in ? __dsub_rn(d0, m0) : 0.0, x1 = in ? __dsub_rn(d1, m1) : 0.0, x2 = in ? __dsub_rn(d2, m2) : 0.0;
    const double c00 = tree_sum(__dmul_rn(x0, x0)), c01 = tree_sum(__dmul_rn(x0, x1)), c02 = tree_sum(__dmul_rn(x0, x2));
    const double c11 = tree_sum(__dmul_rn(x1, x1)), c12 = tree_sum(__dmul_rn(x1, x2)), c22 = tree_sum(__dmul_rn(x2, x2));
    M33 A = {c00, c01, c02, c01, c11, c12, c02, c12, c22}, V = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) jacobi3::sweep(A, V);
    const double a0 = A.m00, a1 = A.m11, a2 = A.m22;
    const bool b1 = a1 < a0;
    const double l1 = b1 ? a1 : a0;
    const bool b2 = a2 < l1;
    const double l = b2 ? a2 : l1;
    const double e0 = b2 ? V.m02 : b1 ? V.m01 : V.m00, e1 = b2 ? V.m12 : b1 ? V.m11 : V.m10, e2 = b2 ? V.m22 : b1 ? V.m21 : V.m20;
    const double nn = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)), __dmul_rn(e2, e2)));
    nx = __ddiv_rn(e0, nn); ny = __ddiv_rn(e1, nn); nz = __ddiv_rn(e2, nn);
    const double w0 = __dsub_rn(vx, px), w1 = __dsub_rn(vy, py), w2 = __dsub_rn(vz, pz);
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(nx, w0), __dmul_rn(ny, w1)), __dmul_rn(nz, w2));
    if (s < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double S = __dadd_rn(__dadd_rn(a0, a1), a2);
    if (l > 0.0 && S > 0.0) cv = __ddiv_rn(l, S);
  }
}

}  // namespace pca
}  // namespace mvicp
