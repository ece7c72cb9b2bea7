// Pieces of the per-cloud structure build shared by the host build (nn_grid.hip build_grid, nn_tile.hip build_wide, nn_mfma.hip build_mfma)
// and the device build (build.hip): the same code runs on both sides, so the two builds make the same bytes.  Every double result that is
// stored goes through b_add / b_sub / b_mul: plain operators on the host, the correctly rounded intrinsics on the device (no contraction).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace mvicp {

struct HashEntry { unsigned long long key; unsigned int start, count; };
struct BrickEntry { unsigned long long mask; unsigned int tab; unsigned int pad; };   // 4x4x4 cells: bit (x&3) | (y&3)<<2 | (z&3)<<4
constexpr unsigned long long kEmptyKey = ~0ull;

__host__ __device__ __forceinline__ double b_add(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dadd_rn(a, b);
#else
  return a + b;
#endif
}
__host__ __device__ __forceinline__ double b_sub(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dsub_rn(a, b);
#else
  return a - b;
#endif
}
__host__ __device__ __forceinline__ double b_mul(double a, double b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}

__host__ __device__ __forceinline__ unsigned long long cell_key(int ix, int iy, int iz) {
  return (unsigned long long)ix | ((unsigned long long)iy << 21) | ((unsigned long long)iz << 42);
}
__host__ __device__ __forceinline__ unsigned int hash_slot(unsigned long long k, int shift) {
  return (unsigned int)((k * 0x9E3779B97F4A7C15ull) >> shift);
}

__host__ __device__ inline unsigned long long morton3(unsigned int x, unsigned int y, unsigned int z) {
  auto spread = [](unsigned long long v) {
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
  };
  return spread(x) | (spread(y) << 1) | (spread(z) << 2);
}

// 3-D Hilbert index of a cell (Skilling's transpose algorithm, `bits` per axis).  Consecutive runs of a Hilbert-sorted
// surface are compact patches without the long jumps of the Z-order curve at power-of-two boundaries, so the boxes of the
// 32-point tiles / 8-ary tree nodes built over the sorted array are tighter and fewer of them overlap a query patch.
__host__ __device__ inline unsigned long long hilbert3(unsigned int x, unsigned int y, unsigned int z, int bits) {
  unsigned int X[3] = {x, y, z};
  const unsigned int M = 1u << (bits - 1);
  for (unsigned int Q = M; Q > 1; Q >>= 1) {
    const unsigned int P = Q - 1;
    for (int i = 0; i < 3; ++i) {
      if (X[i] & Q) X[0] ^= P;
      else { const unsigned int t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
    }
  }
  for (int i = 1; i < 3; ++i) X[i] ^= X[i - 1];
  unsigned int t = 0;
  for (unsigned int Q = M; Q > 1; Q >>= 1) if (X[2] & Q) t ^= Q - 1;
  for (int i = 0; i < 3; ++i) X[i] ^= t;
  return morton3(X[2], X[1], X[0]);   // interleave, X[0] most significant in every bit triple
}

struct HostGrid {
  double o[3], h, inv_h;
  int d[3];
};

__host__ __device__ inline void cell_of(const HostGrid& g, const double* p, int* c) {
  for (int a = 0; a < 3; ++a) {
    int v = (int)floor(b_mul(b_sub(p[a], g.o[a]), g.inv_h));
    c[a] = v < 0 ? 0 : v > g.d[a] - 1 ? g.d[a] - 1 : v;
  }
}

// float bounds of a double, rounded outward (the boxes of the 8-ary tree and of the 64-wide hierarchy)
__host__ __device__ inline float f32_down(double v) { float f = (float)v; if ((double)f > v) f = nextafterf(f, -INFINITY); return f; }
__host__ __device__ inline float f32_up(double v) { float f = (float)v; if ((double)f < v) f = nextafterf(f, INFINITY); return f; }

// f16 pieces of the matrix-pipe operands (exact arithmetic, so the error terms in the block records are maxima, not estimates)
__host__ __device__ inline unsigned short f16_bits(double x) {   // round to nearest even; |x| < 65520 (anything else, NaN included: the largest finite value)
  if (x == 0.0) return 0;
  if (!(fabs(x) < 65520.0)) return (unsigned short)((x < 0 ? 0x8000 : 0) | 0x7bff);
  const unsigned short sign = x < 0 ? 0x8000 : 0;
  const double a = fabs(x);
  int e;
  (void)frexp(a, &e);
  int E = e - 1;
  if (E < -14) return sign | (unsigned short)nearbyint(ldexp(a, 24));   // subnormal: multiples of 2^-24 (1024 -> the smallest normal)
  double k = nearbyint(ldexp(a, 10 - E));
  if (k == 2048.0) { k = 1024.0; ++E; }
  if (E > 15) return sign | 0x7bff;
  return sign | (unsigned short)(((E + 15) << 10) | ((int)k - 1024));
}
__host__ __device__ inline double f16_value(unsigned short h) {
  const int e = (h >> 10) & 31, f = h & 1023;
  const double v = e == 0 ? ldexp((double)f, -24) : ldexp((double)(1024 + f), e - 25);
  return (h & 0x8000) ? -v : v;
}

// the matrix-pipe operands of one target point (nn_mfma.hip): its two 16-B A-fragment rows, and the error terms res (|beta - bt|) and en
// that the block record bounds.  p: the point, c / scale: its block's centre and power-of-two scale; p null: a padding lane.
__host__ __device__ inline void mf_point(const double* p, const double* c, double scale, unsigned short* lo8, unsigned short* hi8, double& res, double& en) {
  for (int a = 0; a < 8; ++a) lo8[a] = hi8[a] = 0;
  hi8[4] = f16_bits(4096.0); hi8[5] = hi8[6] = f16_bits(1.0);
  res = 0.0; en = 0.0;
  if (!p) { lo8[6] = 0x7bff; return; }   // padding: |b|^2 = 65504, never below a finite threshold (and k < n is re-checked before a confirmation)
  double bt[3], res2 = 0.0, nn = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double beta = b_mul(b_sub(p[a], c[a]), scale);
    const unsigned short h = f16_bits(beta);
    const unsigned short l = f16_bits(b_sub(beta, f16_value(h)));
    bt[a] = b_add(f16_value(h), f16_value(l));
    res2 = b_add(res2, b_mul(b_sub(beta, bt[a]), b_sub(beta, bt[a])));
    nn = b_add(nn, b_mul(bt[a], bt[a]));
    lo8[a] = hi8[a] = f16_bits(b_mul(-2.0, f16_value(h)));
    lo8[3 + a] = f16_bits(b_mul(-2.0, f16_value(l)));
  }
  const unsigned short n1 = f16_bits(nn), n2 = f16_bits(b_sub(nn, f16_value(n1))), n3 = f16_bits(b_sub(b_sub(nn, f16_value(n1)), f16_value(n2)));
  lo8[6] = n1; lo8[7] = n2; hi8[3] = n3;
  en = b_add(fabs(b_sub(b_sub(b_sub(nn, f16_value(n1)), f16_value(n2)), f16_value(n3))), b_mul(nn, 1e-15));
  res = sqrt(res2);
}

// the block record's error bound on the fp64 rounding of (p - c) * scale: db = largest res of the block, cloud_max = largest |coordinate|
__host__ __device__ inline float mf_block_db(double db, double cloud_max, const double* c, double scale) {
  return (float)b_add(b_mul(b_add(db, b_mul(b_mul(b_add(b_add(b_add(cloud_max, fabs(c[0])), fabs(c[1])), fabs(c[2])), scale), 4.5e-16)), 1.000001), 1e-30);
}
__host__ __device__ inline float mf_block_en(double en) { return (float)b_add(b_mul(en, 1.000001), 1e-30); }

// ---- host-only steps that both builds run as they are ----------------------------------------------------------------------------------

inline void make_grid(HostGrid& g, const double* lo, const double* hi, double h) {
  g.h = h; g.inv_h = 1.0 / h;
  for (int a = 0; a < 3; ++a) {
    g.o[a] = lo[a] - 0.01 * h;
    g.d[a] = std::max(1, (int)std::ceil((hi[a] - g.o[a]) * g.inv_h + 0.01) + 1);
    g.d[a] = std::min(g.d[a], (1 << 21) - 1);
  }
}

// cell edge: aim at ~`target` points per occupied cell.  Measure occupancy at two resolutions (the cloud is a surface, so occupied(h) ~ h^-dim
// with dim ~ 2), extrapolate, verify once.  occupied(g) = number of distinct cells of the cloud's points (at most 5 calls).  Returns 0 or the
// first failing status of occupied (reported as a negative count).
template <typename Occ>
int choose_grid(HostGrid& g, int n, const double* lo, const double* hi, double target, Occ&& occupied) {
  double ext = std::max(std::max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
  if (!(ext > 0.0)) ext = 1.0;
  double h = ext / std::max(2.0, std::cbrt((double)n));
  if (n > 64) {
    long long o;
    make_grid(g, lo, hi, h);
    if ((o = occupied(g)) < 0) return (int)o;
    const double occ1 = (double)o;
    make_grid(g, lo, hi, 2.0 * h);
    if ((o = occupied(g)) < 0) return (int)o;
    const double occ2 = (double)o;
    double dim = std::log(std::max(occ1, 1.0) / std::max(occ2, 1.0)) / std::log(2.0);
    dim = std::min(3.0, std::max(1.0, dim));
    const double want = (double)n / target;
    h = h * std::pow(std::max(occ1, 1.0) / want, 1.0 / dim);
    h = std::min(std::max(h, ext * 1e-6), ext);
    for (int it = 0; it < 3; ++it) {
      make_grid(g, lo, hi, h);
      if ((o = occupied(g)) < 0) return (int)o;
      const double per = (double)n / (double)o;
      if (per < 0.6 * target) h *= std::pow(target / per, 1.0 / dim);
      else if (per > 1.8 * target) h *= std::pow(target / per, 1.0 / dim);
      else break;
    }
  }
  make_grid(g, lo, hi, h);
  return 0;
}

// bits per axis of the Hilbert curve over the grid
inline int curve_bits(const HostGrid& g) {
  int hbits = 1;
  while ((1 << hbits) < std::max(g.d[0], std::max(g.d[1], g.d[2]))) ++hbits;
  return hbits;
}

// open-addressing hash of the cell runs, inserted in run order (the linear-probing layout depends on it)
inline void hash_runs(const std::vector<HashEntry>& runs, std::vector<HashEntry>& table, unsigned int& mask, int& shift) {
  int log2size = 4;
  while ((1ull << log2size) < 2 * runs.size() + 2) ++log2size;
  const unsigned int tsize = 1u << log2size;
  mask = tsize - 1;
  shift = 64 - log2size;
  table.assign(tsize, HashEntry{kEmptyKey, 0u, 0u});
  for (const HashEntry& r : runs) {
    unsigned int s = hash_slot(r.key, shift);
    while (table[s].key != kEmptyKey) s = (s + 1) & mask;
    table[s] = r;
  }
}

// dense brick map (nn_cell_kernel): 4x4x4-cell bricks -> occupancy mask + row of the cell table; cell table = {start, count} of
// every cell run.  Only built when the dense array stays small (a surface scan at a few points per cell: ~1e5..1e6 bricks) and the
// hash runs index the canonical arrays (nn_cell_kernel stages runs of them).  Returns false when there is none.
inline bool brick_map(const std::vector<HashEntry>& runs, const HostGrid& g, int n, bool split_orders, std::vector<BrickEntry>& bricks,
                      std::vector<uint2>& celltab, int* bdims) {
  const long long bd[3] = {(g.d[0] + 3) / 4, (g.d[1] + 3) / 4, (g.d[2] + 3) / 4};
  const long long nb = bd[0] * bd[1] * bd[2];
  const bool capped = g.d[0] >= (1 << 21) - 1 || g.d[1] >= (1 << 21) - 1 || g.d[2] >= (1 << 21) - 1;
  if (split_orders || capped || nb > (1ll << 24) || n >= (1 << 30)) return false;
  bricks.assign((size_t)nb, BrickEntry{0ull, 0xffffffffu, 0u});
  celltab.clear();
  unsigned int n_tab = 0;
  for (const HashEntry& r : runs) {
    const int ix = (int)(r.key & 0x1fffffull), iy = (int)((r.key >> 21) & 0x1fffffull), iz = (int)((r.key >> 42) & 0x1fffffull);
    BrickEntry& be = bricks[(size_t)(((long long)(iz >> 2) * bd[1] + (iy >> 2)) * bd[0] + (ix >> 2))];
    if (be.tab == 0xffffffffu) { be.tab = n_tab++; celltab.resize((size_t)n_tab * 64, make_uint2(0u, 0u)); }
    const int bit = (ix & 3) | ((iy & 3) << 2) | ((iz & 3) << 4);
    be.mask |= 1ull << bit;
    celltab[(size_t)be.tab * 64 + bit] = make_uint2(r.start, r.count);
  }
  bdims[0] = (int)bd[0]; bdims[1] = (int)bd[1]; bdims[2] = (int)bd[2];
  return true;
}

// shape of the implicit complete 8-ary box tree: of the (depth, leaf size) pairs that cover n the one with the fewest empty leaves
inline void oct_shape(int n, int& D8, int& L8) {
  D8 = 0; L8 = 8;
  long long best_cap = -1;
  for (int d = 0; d <= 7; ++d)      // OCT_STACK holds 7 entries per level + 1
    for (int l8 = 8; l8 <= 32; l8 *= 2) {
      const long long cap = (1ll << (3 * d)) * l8;
      if (cap >= std::max(n, 1) && (best_cap < 0 || cap < best_cap)) { best_cap = cap; D8 = d; L8 = l8; }
    }
  if (best_cap < 0) { D8 = 7; L8 = 64; while ((1ll << 21) * L8 < n) L8 *= 2; }   // > 67 M points: longer leaves
}

}  // namespace mvicp
