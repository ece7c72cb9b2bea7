// The pieces of descriptor matching that must be the same bits wherever they run: the best-two list of a row and the tile loops of the two
// kernels of match.hip.  match.hip and coarse.hip both include this file, so there is one statement of the arithmetic.  DESIGN.md §3.11, §3.12.
#pragma once
#include "common.h"

namespace mvicp {
namespace match_tile {

constexpr int kThreads = 256;   // left rows per workgroup of the register kernel
constexpr int kTile = 64;       // right rows per LDS tile
constexpr int kGenRows = 64;    // left rows per workgroup of the generic kernel
constexpr int kGenTile = 32;    // its right rows per LDS tile
constexpr int kMaxDim = 64;

struct Best2 { double d0, d1; int j0, j1; };   // the first two of a row in (d2, j) order; j < 0: the slot is empty (d = +inf)
static_assert(sizeof(Best2) == 24, "Best2 is 24 bytes");

// candidates arrive in ascending j (or chunk by chunk in ascending j, each chunk's own two in order): a strict comparison keeps the lower j
__device__ __forceinline__ void offer(double d, int j, double& d0, int& j0, double& d1, int& j1) {
  const bool first = j0 < 0 || d < d0, second = !first && (j1 < 0 || d < d1);   // (selects: the four values stay in registers)
  d1 = first ? d0 : second ? d : d1; j1 = first ? j0 : second ? j : j1;
  d0 = first ? d : d0; j0 = first ? j : j0;
}

template <int DIM> struct RegTile { static constexpr int LD = DIM + (DIM & 1); };   // (an even row length keeps every row 16-byte aligned)

// rows lo .. hi of B against row i of A held in registers (live: the row exists); Bs: kTile * RegTile<DIM>::LD doubles of LDS; every
// thread of the workgroup of kThreads calls it.  j counts from B's first row.
template <int DIM>
__device__ __forceinline__ void scan_reg(const double* __restrict__ A, long long i, bool live, const double* __restrict__ B, long long lo, long long hi,
                                         double* Bs, double& d0, int& j0, double& d1, int& j1) {
  constexpr int LD = RegTile<DIM>::LD;
  constexpr int SEG = 11;               // the early-exit check follows each sub-histogram
  static_assert(DIM % SEG == 0, "the row is a whole number of segments");
  double a[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) a[c] = live ? A[(size_t)i * DIM + c] : 0.0;
  for (long long base = lo; base < hi; base += kTile) {
    const int rows = (int)(hi - base < kTile ? hi - base : kTile);
    __syncthreads();   // (the last tile has been read by every wave)
    for (int e = threadIdx.x; e < rows * DIM; e += kThreads) {
      const int r = e / DIM, c = e - r * DIM;
      Bs[r * LD + c] = B[(size_t)base * DIM + e];
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double* b = Bs + r * LD;
      double s = 0.0;
      bool skip = false;
#pragma unroll
      for (int g = 0; g < DIM / SEG; ++g) {
#pragma unroll
        for (int c = g * SEG; c < (g + 1) * SEG; ++c) {
          const double t = __dsub_rn(a[c], b[c]);
          s = __dadd_rn(s, __dmul_rn(t, t));
        }
        // s only grows from here: above the second best (never above an empty slot's +inf) it cannot enter
        if (g + 1 < DIM / SEG && __all(!live || s > d1)) { skip = true; break; }
      }
      if (!skip) offer(s, (int)(base + r), d0, j0, d1, j1);
    }
  }
}

// rows lo .. hi of B against the kGenRows rows of A from i0 on (m rows in all); As: kMaxDim * kGenRows doubles of LDS ([c][row]), Bs:
// kGenTile * kMaxDim ([row][c]); every thread of the workgroup of kGenRows calls it and owns row i0 + threadIdx.x
__device__ __forceinline__ void scan_generic(const double* __restrict__ A, int m, long long i0, const double* __restrict__ B, long long lo, long long hi,
                                             int dim, double* As, double* Bs, double& d0, int& j0, double& d1, int& j1) {
  const int rows_a = (int)((long long)m - i0 < kGenRows ? (long long)m - i0 : kGenRows);
  for (int e = threadIdx.x; e < kGenRows * dim; e += kGenRows) {
    const int r = e / dim, c = e - r * dim;
    As[c * kGenRows + r] = r < rows_a ? A[(size_t)i0 * dim + e] : 0.0;
  }
  for (long long base = lo; base < hi; base += kGenTile) {
    const int rows = (int)(hi - base < kGenTile ? hi - base : kGenTile);
    __syncthreads();
    for (int e = threadIdx.x; e < rows * dim; e += kGenRows) Bs[e] = B[(size_t)base * dim + e];
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const double* b = Bs + r * dim;
      double s = 0.0;
      for (int c = 0; c < dim; ++c) {
        const double t = __dsub_rn(As[c * kGenRows + threadIdx.x], b[c]);
        s = __dadd_rn(s, __dmul_rn(t, t));
      }
      offer(s, (int)(base + r), d0, j0, d1, j1);
    }
  }
}

// the best two of one row over its `chunks` partial lists, chunk y of row i at part[y * rows + i]
__device__ __forceinline__ void merge_row(const Best2* __restrict__ part, size_t rows, size_t i, int chunks, double& d0, int& j0, double& d1, int& j1) {
  for (int y = 0; y < chunks; ++y) {
    const Best2* p = part + ((size_t)y * rows + i);
    const double pd0 = p->d0, pd1 = p->d1; const int pj0 = p->j0, pj1 = p->j1;
    if (pj0 >= 0) offer(pd0, pj0, d0, j0, d1, j1);
    if (pj1 >= 0) offer(pd1, pj1, d0, j0, d1, j1);
  }
}

}  // namespace match_tile
}  // namespace mvicp
