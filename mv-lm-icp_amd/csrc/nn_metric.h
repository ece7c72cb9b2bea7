// The rounded operations every exact NN kernel shares (brute, grid, tile, matrix-pipe, tie fix-up, normals, overlap): the query transform of
// Frame::computeClosestPointsToNeighbours (frame.cpp:117-118,131,136), the reference metric (frame.h:70-76, no fma) and the lower
// bound of a query to an outward-rounded float box of the implicit 8-ary tree, evaluated in the SAME rounded operations as the
// point distance (every rounding is monotone, so lb <= d2 for every point inside the box: DESIGN.md §3.4).
#pragma once
#include <hip/hip_runtime.h>

namespace mvicp {

constexpr int OCT_STACK = 56;  // entries of an octet's descent stack: >= 7 * max depth + 1 (build_grid keeps the depth <= 7)

// x = the rigid part of an edge's kEdgeXf (common.h, kXfRigid doubles): Rs(9) ts(3) Rd^-1(9) td(3), column-major
// g_i = ((R(i,0) p0 + R(i,1) p1) + R(i,2) p2) + t_i ; u = g - t_d ; q_i = (Ri(i,0) u0 + Ri(i,1) u1) + Ri(i,2) u2
__device__ __forceinline__ void xf_point(const double* __restrict__ x, double p0, double p1, double p2, double& q0, double& q1, double& q2) {
  double g[3], u[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    g[i] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(x[i], p0), __dmul_rn(x[i + 3], p1)), __dmul_rn(x[i + 6], p2)), x[9 + i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = __dsub_rn(g[i], x[21 + i]);
  q0 = __dadd_rn(__dadd_rn(__dmul_rn(x[12 + 0], u[0]), __dmul_rn(x[12 + 3], u[1])), __dmul_rn(x[12 + 6], u[2]));
  q1 = __dadd_rn(__dadd_rn(__dmul_rn(x[12 + 1], u[0]), __dmul_rn(x[12 + 4], u[1])), __dmul_rn(x[12 + 7], u[2]));
  q2 = __dadd_rn(__dadd_rn(__dmul_rn(x[12 + 2], u[0]), __dmul_rn(x[12 + 5], u[1])), __dmul_rn(x[12 + 8], u[2]));
}

__device__ __forceinline__ double dist2(double qx, double qy, double qz, double x, double y, double z) {
  const double d0 = __dsub_rn(qx, x), d1 = __dsub_rn(qy, y), d2 = __dsub_rn(qz, z);
  return __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2));
}

__device__ __forceinline__ double oct_box_lb(double qx, double qy, double qz, const float4 a, const float4 b) {
  // box = {lo.xyz = a.xyz, hi.xyz = (a.w, b.x, b.y)}
  const double g0 = fmax(fmax(__dsub_rn((double)a.x, qx), __dsub_rn(qx, (double)a.w)), 0.0);
  const double g1 = fmax(fmax(__dsub_rn((double)a.y, qy), __dsub_rn(qy, (double)b.x)), 0.0);
  const double g2 = fmax(fmax(__dsub_rn((double)a.z, qz), __dsub_rn(qz, (double)b.y)), 0.0);
  return __dadd_rn(__dadd_rn(__dmul_rn(g0, g0), __dmul_rn(g1, g1)), __dmul_rn(g2, g2));
}

}  // namespace mvicp
