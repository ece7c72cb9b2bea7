// FPFH surface descriptors (mvicp_fpfh): the 33-bin Fast Point Feature Histogram of every point of one stored cloud with normals, as a
// pure function of the stored bytes, bit for bit.  The contract is stated in include/mvicp.h; tests/fpfhref.py is its numpy form and its
// scalar-loop form.  DESIGN.md §3.10.
//
// The neighbourhoods are the rows of one internal knn_search (self mode, hybrid: the max_nn nearest within the radius, ordered by
// (dist2, original index)); a row is at most 64 long, one wave64.  Two passes behind it, on the context's stream:
//   1  fpfh_spfh  one wave per point, lane t = entry t of the row: the pair's three bins in fp64 (+ - x / sqrt, comparisons and floor
//                 only, every operation rounded on its own), the 33 counts by ballot + popcount per bin (integers: no order to keep),
//                 stored as a 48-byte record {33 count bytes, zero padding, r = 100 / m}
//   2  fpfh_sum   one wave per point, lane b = bin b: lane t first forms g = r_j / d2 of entry t (one division per neighbour), then the
//                 wave walks the row IN ORDER -- the order of the additions is part of the contract -- eight neighbours' count bytes in
//                 flight at a time, g broadcast from lane t; then the three sub-histogram sums in ascending bin order (no tree) and the row.
// Bytes rather than doubles in the records keep the gather of pass 2 at one 48-byte record per neighbour instead of 264 bytes.
#include "common.h"

namespace mvicp {

namespace {

constexpr int kBins = 33;
constexpr int kWavesPerBlock = 4;
constexpr int kInFlight = 8;   // neighbours whose count bytes pass 2 has in flight

struct SpfhRec { unsigned char c[40]; double r; };   // counts 0 .. 32, zero padding, r = 100 / m (0: m == 0)
static_assert(sizeof(SpfhRec) == 48, "SpfhRec is 48 bytes");

// the doubles nearest to cos / sin of the inner edges phi_k = -pi + 2 pi k / 11, k = 1 .. 10; the same literals as tests/fpfhref.py
__device__ const double kEdgeC[10] = {-0x1.aeb8c8764f0bap-1, -0x1.a9628d9c712b6p-2, 0x1.2375f640f44dbp-3, 0x1.4f49e7f775887p-1, 0x1.eb42a9bcd5057p-1,
                                      0x1.eb42a9bcd5057p-1, 0x1.4f49e7f775887p-1, 0x1.2375f640f44dbp-3, -0x1.a9628d9c712b6p-2, -0x1.aeb8c8764f0bap-1};
__device__ const double kEdgeS[10] = {-0x1.14cedf8bb580bp-1, -0x1.d1bb48eee2c13p-1, -0x1.fac9e043842efp-1, -0x1.82f19bb3a28a1p-1, -0x1.207e7fd768dbfp-2,
                                      0x1.207e7fd768dbfp-2, 0x1.82f19bb3a28a1p-1, 0x1.fac9e043842efp-1, 0x1.d1bb48eee2c13p-1, 0x1.14cedf8bb580bp-1};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
  return __dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz));
}
__device__ __forceinline__ double cross1(double a1, double a2, double b1, double b2) { return __dsub_rn(__dmul_rn(a1, b2), __dmul_rn(a2, b1)); }

__device__ __forceinline__ int bin11(double f) {
  const double t = floor(__dmul_rn(__dadd_rn(f, 1.0), 5.5));
  return (int)fmin(fmax(t, 0.0), 10.0);
}

// the number of inner edges the angle of (x, y) in (-pi, pi] has passed
__device__ __forceinline__ int theta_bin(double x, double y) {
  int b = 0;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const double cr = __dsub_rn(__dmul_rn(kEdgeC[k], y), __dmul_rn(kEdgeS[k], x));
    const bool passed = k < 5 ? (y >= 0.0 || cr >= 0.0) : ((y > 0.0 && cr >= 0.0) || (y == 0.0 && x < 0.0));
    b += passed ? 1 : 0;
  }
  return b;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {   // lane is wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void fpfh_spfh_kernel(const double* __restrict__ pts, const double* __restrict__ nor, int n, int k,
                                                                        const int* __restrict__ cnt, const int* __restrict__ idx,
                                                                        const double* __restrict__ d2, SpfhRec* __restrict__ rec, int* __restrict__ used) {
  // (one wave per point: saying so lets the point's own loads and the loop bounds be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];   // <= k <= 64
  bool valid = false;
  int b0 = 0, b1 = 0, b2 = 0;
  if (lane < len) {
    const size_t e = (size_t)i * (size_t)k + lane;
    const double dd = d2[e];
    if (dd != 0.0) {   // the point itself and exact duplicates: no pair frame
      valid = true;
      const double* pi = pts + 3 * (size_t)i; const double* ni = nor + 3 * (size_t)i;
      const size_t j = (size_t)idx[e];
      const double* pj = pts + 3 * j; const double* nj = nor + 3 * j;
      const double nix = ni[0], niy = ni[1], niz = ni[2], njx = nj[0], njy = nj[1], njz = nj[2];
      const double dx = __dsub_rn(pj[0], pi[0]), dy = __dsub_rn(pj[1], pi[1]), dz = __dsub_rn(pj[2], pi[2]);
      const double dist = __dsqrt_rn(dd);
      const double a1 = dot3(nix, niy, niz, dx, dy, dz), a2 = dot3(njx, njy, njz, dx, dy, dz);
      const bool swap = fabs(a1) < fabs(a2);
      const double sx = swap ? njx : nix, sy = swap ? njy : niy, sz = swap ? njz : niz;
      const double tx = swap ? nix : njx, ty = swap ? niy : njy, tz = swap ? niz : njz;
      const double ex = swap ? -dx : dx, ey = swap ? -dy : dy, ez = swap ? -dz : dz;
      const double f3 = __ddiv_rn(swap ? -a2 : a1, dist);
      double vx = cross1(ey, ez, sy, sz), vy = cross1(ez, ex, sz, sx), vz = cross1(ex, ey, sx, sy);
      const double vn = __dsqrt_rn(dot3(vx, vy, vz, vx, vy, vz));
      if (vn == 0.0) {
        b0 = b1 = b2 = 5;
      } else {
        vx = __ddiv_rn(vx, vn); vy = __ddiv_rn(vy, vn); vz = __ddiv_rn(vz, vn);
        const double wx = cross1(sy, sz, vy, vz), wy = cross1(sz, sx, vz, vx), wz = cross1(sx, sy, vx, vy);
        const double f2 = dot3(vx, vy, vz, tx, ty, tz);
        const double y = dot3(wx, wy, wz, tx, ty, tz), x = dot3(sx, sy, sz, tx, ty, tz);
        b0 = theta_bin(x, y); b1 = bin11(f2); b2 = bin11(f3);
      }
    }
  }
  // lane b < 33 ends up with count b: one ballot per bin (integers, so any way of counting is exact)
  int mine = 0;
#pragma unroll
  for (int b = 0; b < 11; ++b) {
    const int c0 = __popcll(__ballot(valid && b0 == b)), c1 = __popcll(__ballot(valid && b1 == b)), c2 = __popcll(__ballot(valid && b2 == b));
    mine = lane == b ? c0 : lane == 11 + b ? c1 : lane == 22 + b ? c2 : mine;
  }
  const int m = __popcll(__ballot(valid));   // <= 63
  if (lane < 40) rec[i].c[lane] = (unsigned char)mine;   // (lanes 33 .. 39: the zero padding)
  if (lane == 40) rec[i].r = m ? __ddiv_rn(100.0, (double)m) : 0.0;
  if (lane == 41) used[i] = m;
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void fpfh_sum_kernel(int n, int k, const int* __restrict__ cnt, const int* __restrict__ idx,
                                                                       const double* __restrict__ d2, const SpfhRec* __restrict__ rec,
                                                                       double* __restrict__ desc) {
  // (one wave per point: saying so lets the point's own loads and the loop bounds be scalar)
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6))), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int len = cnt[i];
  // lane t: neighbour j and weight g of entry t.  The entries with d2 == 0 are a prefix of the row (it ascends in d2), so N(i) is the
  // lanes [zeros, len)
  int j = i; double g = 0.0; bool zero = false;
  if (lane < len) {
    const size_t e = (size_t)i * (size_t)k + lane;
    const double dd = d2[e];
    zero = dd == 0.0;
    if (!zero) { j = idx[e]; g = __ddiv_rn(rec[j].r, dd); }
  }
  const int zeros = __popcll(__ballot(zero));
  const int bl = lane < 40 ? lane : 0;   // the byte this lane reads of every record (lanes >= 33 carry nothing that is stored)
  double acc = 0.0;
  for (int base = zeros; base < len; base += kInFlight) {
    unsigned char cb[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int jt = __builtin_amdgcn_readlane(j, min(base + u, len - 1));
      cb[u] = rec[jt].c[bl];
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u)
      if (base + u < len) acc = __dadd_rn(acc, __dmul_rn((double)cb[u], readlane_f64(g, base + u)));
  }
  // the three sub-histogram sums, each over its 11 bins in ascending order
  double S[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < 11; ++b) s = __dadd_rn(s, readlane_f64(acc, 11 * f + b));
    S[f] = s;
  }
  if (lane >= kBins) return;
  const double Sf = lane < 11 ? S[0] : lane < 22 ? S[1] : S[2];
  const double scale = Sf != 0.0 ? __ddiv_rn(100.0, Sf) : 0.0;
  const double own = __dmul_rn((double)rec[i].c[lane], rec[i].r);
  desc[(size_t)i * kBins + lane] = __dadd_rn(__dmul_rn(acc, scale), own);
}

}  // namespace

long long fpfh_compute(mvicp_ctx* c, const FrameDev& f, int max_nn, double radius, double B2) {
  c->fpfh.rows = -1;   // (the last result ends here; a failed call leaves none behind)
  const long long total = knn_search(c, f, nullptr, 0, 0, max_nn, radius, B2);
  if (total < 0) return total;
  const int n = f.n;
  if (n == 0) { c->fpfh.rows = 0; return 0; }
  hipStream_t st = c->stream;
  const size_t N = (size_t)n;
  const size_t off_used = align256(8 * kBins * N), off_rec = off_used + align256(4 * N), need = off_rec + align256(sizeof(SpfhRec) * N);
  MV_CHECK(c->fpfh.dev.reserve(need));
  c->fpfh.desc = reinterpret_cast<double*>(c->fpfh.dev.p);
  c->fpfh.used = reinterpret_cast<int*>(c->fpfh.dev.p + off_used);
  SpfhRec* rec = reinterpret_cast<SpfhRec*>(c->fpfh.dev.p + off_rec);
  const dim3 grid((unsigned int)((N + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
  const double row_bytes = 4.0 + 12.0 * max_nn;   // cnt and the dense row (idx, d2) of a point
  {
    // per point its position, normal, row and record; per neighbour a position and a normal
    ProfScope ps(c, "fpfh_spfh", (48.0 + row_bytes + sizeof(SpfhRec) + 4.0) * n + 48.0 * total);
    hipLaunchKernelGGL(fpfh_spfh_kernel, grid, block, 0, st, f.pts, f.nor, n, max_nn, c->knn.cnt, c->knn.idx, c->knn.d2, rec, c->fpfh.used);
    MV_HIP(hipGetLastError());
  }
  {
    // per point its row, its own 33 counts and r, the 33 doubles it writes; per neighbour 33 count bytes and r
    ProfScope ps(c, "fpfh_sum", (row_bytes + 41.0 + 8.0 * kBins) * n + 41.0 * total);
    hipLaunchKernelGGL(fpfh_sum_kernel, grid, block, 0, st, n, max_nn, c->knn.cnt, c->knn.idx, c->knn.d2, rec, c->fpfh.desc);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipStreamSynchronize(st));
  c->fpfh.rows = n;
  return n;
}

}  // namespace mvicp
