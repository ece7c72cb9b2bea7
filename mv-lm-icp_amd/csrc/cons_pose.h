// The pieces of the consensus pose that must be the same bits wherever they run: the sampler, the triangle frame, the hypothesis and the
// inlier test.  consensus.hip and coarse.hip both include this file, so there is one statement of the arithmetic.  DESIGN.md §3.11, §3.12.
#pragma once
#include "common.h"

namespace mvicp {
namespace cons_pose {

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}
__device__ __forceinline__ double cross1(double a1, double a2, double b1, double b2) { return __dsub_rn(__dmul_rn(a1, b2), __dmul_rn(a2, b1)); }

__device__ __forceinline__ unsigned long long sample_index(unsigned long long seed, unsigned int h, int t, unsigned long long c) {
  unsigned long long z = seed + (3ull * h + (unsigned long long)t + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  const unsigned long long u = z ^ (z >> 31);
  return ((u >> 32) * c) >> 32;
}

// the orthonormal frame (e1, e2, e3) of the triangle T (three points, 9 doubles); false: a degenerate triangle
__device__ __forceinline__ bool tri_frame(const double* T, double* e1, double* e2, double* e3) {
  const double ux = __dsub_rn(T[3], T[0]), uy = __dsub_rn(T[4], T[1]), uz = __dsub_rn(T[5], T[2]);
  const double n1 = __dsqrt_rn(dot3(ux, uy, uz, ux, uy, uz));
  if (n1 == 0.0) return false;
  e1[0] = __ddiv_rn(ux, n1); e1[1] = __ddiv_rn(uy, n1); e1[2] = __ddiv_rn(uz, n1);
  const double vx = __dsub_rn(T[6], T[0]), vy = __dsub_rn(T[7], T[1]), vz = __dsub_rn(T[8], T[2]);
  const double wx = cross1(e1[1], e1[2], vy, vz), wy = cross1(e1[2], e1[0], vz, vx), wz = cross1(e1[0], e1[1], vx, vy);
  const double nw = __dsqrt_rn(dot3(wx, wy, wz, wx, wy, wz));
  if (nw == 0.0) return false;
  e3[0] = __ddiv_rn(wx, nw); e3[1] = __ddiv_rn(wy, nw); e3[2] = __ddiv_rn(wz, nw);
  e2[0] = cross1(e3[1], e3[2], e1[1], e1[2]); e2[1] = cross1(e3[2], e3[0], e1[2], e1[0]); e2[2] = cross1(e3[0], e3[1], e1[0], e1[1]);
  return true;
}

// hypothesis h: accepted?  With WANT_POSE also R (row-major) and t
template <bool WANT_POSE>
__device__ __forceinline__ bool hypothesis(const double* __restrict__ P, const double* __restrict__ Q, unsigned long long c, unsigned long long seed,
                                           unsigned int h, double s2, double* R, double* t) {
  const unsigned long long i0 = sample_index(seed, h, 0, c), i1 = sample_index(seed, h, 1, c), i2 = sample_index(seed, h, 2, c);
  if (i0 == i1 || i1 == i2 || i2 == i0) return false;
  double TP[9], TQ[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    TP[k] = P[3 * i0 + k]; TP[3 + k] = P[3 * i1 + k]; TP[6 + k] = P[3 * i2 + k];
    TQ[k] = Q[3 * i0 + k]; TQ[3 + k] = Q[3 * i1 + k]; TQ[6 + k] = Q[3 * i2 + k];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {   // the edges (0,1), (1,2), (2,0)
    const int a = 3 * e, b = 3 * ((e + 1) % 3);
    const double px = __dsub_rn(TP[a], TP[b]), py = __dsub_rn(TP[a + 1], TP[b + 1]), pz = __dsub_rn(TP[a + 2], TP[b + 2]);
    const double qx = __dsub_rn(TQ[a], TQ[b]), qy = __dsub_rn(TQ[a + 1], TQ[b + 1]), qz = __dsub_rn(TQ[a + 2], TQ[b + 2]);
    const double lp = dot3(px, py, pz, px, py, pz), lq = dot3(qx, qy, qz, qx, qy, qz);
    if (!(lp >= __dmul_rn(s2, lq) && lq >= __dmul_rn(s2, lp))) return false;
  }
  double e1[3], e2[3], e3[3], f1[3], f2[3], f3[3];
  if (!tri_frame(TP, e1, e2, e3) || !tri_frame(TQ, f1, f2, f3)) return false;
  if (WANT_POSE) {
    double cp[3], cq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cp[k] = __ddiv_rn(__dadd_rn(__dadd_rn(TP[k], TP[3 + k]), TP[6 + k]), 3.0);
      cq[k] = __ddiv_rn(__dadd_rn(__dadd_rn(TQ[k], TQ[3 + k]), TQ[6 + k]), 3.0);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) R[3 * r + k] = __dadd_rn(__dadd_rn(__dmul_rn(f1[r], e1[k]), __dmul_rn(f2[r], e2[k])), __dmul_rn(f3[r], e3[k]));
      t[r] = __dsub_rn(cq[r], dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], cp[0], cp[1], cp[2]));
    }
  }
  return true;
}

__device__ __forceinline__ bool inlier(const double* R, const double* t, const double* p, const double* q, double tau2) {
  const double rx = __dsub_rn(__dadd_rn(dot3(R[0], R[1], R[2], p[0], p[1], p[2]), t[0]), q[0]);
  const double ry = __dsub_rn(__dadd_rn(dot3(R[3], R[4], R[5], p[0], p[1], p[2]), t[1]), q[1]);
  const double rz = __dsub_rn(__dadd_rn(dot3(R[6], R[7], R[8], p[0], p[1], p[2]), t[2]), q[2]);
  return dot3(rx, ry, rz, rx, ry, rz) <= tau2;
}

}  // namespace cons_pose
}  // namespace mvicp
