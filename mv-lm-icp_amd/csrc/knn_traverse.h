// The growing-block traversal of the per-cloud hash, written once for every kernel that asks "which points of this cloud lie around this
// point" (knn.hip: the k-nearest and radius searches; iss.hip: the keypoint moments and the non-maximum suppression; outlier.hip: the
// k+1 smallest distances; normals.hip: the reference-parity k-NN lists): the views of the structures it reads and traverse() itself, with
// every exactness argument (the face bound, the 0.999 margin, the 2 n rule).  The hash's small parts are build_common.h's.  offer gets the
// candidate's record, so a caller that needs the neighbour's coordinates reads them from the registers the distance was computed from,
// and one that needs its cell-order position takes record - g.crec (valid without a tree: a tree leaf's records are in sorted order).
#pragma once
#include "build_common.h"
#include "common.h"
#include "nn_metric.h"

namespace mvicp {

namespace {
constexpr int kTreeAfter = 4;   // a block of this radius (9^3 cells) that has not finished hands the query to the box tree

struct GridView {
  const PointRec* crec; int n;   // records in hash-CELL order
  const HashEntry* table; unsigned int mask; int shift;
  double ox, oy, oz, h, inv_h;
  int dx, dy, dz;
};

// the implicit 8-ary box tree of nn_grid.hip over the records in sorted order.  It lives in device memory next to the control block and is
// read only by a lane that walks the tree, after its block loop: as kernel arguments these words would be live across the whole loop nest
// (measured: 8 spilled SGPRs in every build of the search kernel)
struct TreeView { const PointRec* srec; const float* oct; long long first_leaf; int leaf, pad; };

// host: the view of a built cloud's hash; n = the cloud's points
inline void fill_grid_view(GridView* v, const GridDev& g, int n) {
  v->crec = (const PointRec*)g.crec; v->n = n;
  v->table = (const HashEntry*)g.table; v->mask = g.table_mask; v->shift = g.table_shift;
  v->ox = g.origin[0]; v->oy = g.origin[1]; v->oz = g.origin[2]; v->h = g.cell; v->inv_h = g.inv_cell;
  v->dx = g.dims[0]; v->dy = g.dims[1]; v->dz = g.dims[2];
}

// host: the view of the cloud's box tree, staged through the caller's pinned slot h_slot into its device slot d_slot (queued on st; the
// pinned slot must not be in flight: every call of a stage waits for its work).  *out = d_slot, or stays as it is for a cloud without a tree
inline int stage_tree_view(const GridDev& g, void* h_slot, void* d_slot, hipStream_t st, const TreeView** out) {
  if (!g.oct || !g.srec) return MVICP_OK;
  TreeView* h_tree = reinterpret_cast<TreeView*>(h_slot);
  h_tree->srec = (const PointRec*)g.srec; h_tree->oct = g.oct; h_tree->first_leaf = g.oct_first_leaf; h_tree->leaf = g.oct_leaf; h_tree->pad = 0;
  MV_HIP(hipMemcpyAsync(d_slot, h_tree, sizeof(TreeView), hipMemcpyHostToDevice, st));
  *out = reinterpret_cast<const TreeView*>(d_slot);
  return MVICP_OK;
}

// the clamped home cell along one axis; clamped as a double, so that a query far outside the grid cannot overflow the conversion
__device__ __forceinline__ int home_cell(double q, double o, double inv_h, int d) {
  return (int)fmin(fmax(floor((q - o) * inv_h), 0.0), (double)(d - 1));
}

// The growing block around the query's clamped home cell: offer(d2, record) for every point of every cell, each point once; after
// every block stop(m2) with m2 = the square of a lower bound on the distance from the query to every point NOT yet offered.  Returns when
// stop says so or every point has been offered.  Two ways out of a block that keeps growing through empty cells, both after reset() (the
// caller forgets what was offered, because everything is offered again):
//   * the block exceeded 2 n cells (a small cloud in a sparse grid): the cloud itself is offered, O(n), exact by construction;
//   * the block of radius kTreeAfter has not finished (a query in empty space: a probe off the surface, a point of a far cluster): a
//     depth-first walk of the implicit 8-ary box tree of nn_grid.hip, one lane per query and stackless (first child 8 id + 1, next
//     sibling id + 1, parent (id - 1) / 8), which opens a box only if open(lb) -- lb = oct_box_lb, a lower bound on the COMPUTED dist2
//     of every point in the box (the boxes are rounded outwards and every operation of dist2 is monotone) -- and offers the points of
//     the leaves it opens.  Without it a query in empty space costs O(r^3) cell look-ups and then O(n) points.
//
// face_bound.  The block of radius r holds the cells [c - r, c + r] per axis, clamped to the grid.  A point that is not in the block lies
// in a cell outside that range along at least one axis, on one side of it; it is then beyond the block's face on that side, and its
// distance to the query is at least the query's distance to that face's plane, PROVIDED the query is on the inner side of the plane.
//   * A face that coincides with the grid boundary (c - r <= 0 on the low side, c + r >= d - 1 on the high side) has no cell beyond it,
//     so no point is "outside the block on that side" and the face does not enter the minimum.  (With all six faces a query outside
//     the grid would never stop early: the clamped home cell makes the boundary face's term <= 0.  One of the cloud's own points merely
//     stops a block sooner without it.)
//   * For every other face the query is on the inner side: on the low side c - r > 0 implies c > 0, so the home cell was not clamped from
//     below and q >= o + c h >= o + (c - r) h + h (up to the rounding of the cell assignment); a query beyond the HIGH grid boundary has
//     c = d - 1 and is even farther from every low face.  The high side mirrors this.  So the existing expressions q - f and f + w - q are
//     each >= h (1 - rounding) > 0 and valid lower bounds, and the 0.999 margin absorbs the rounding as it does in normals.hip.
//   * No face left: the block covers the grid and every point has been offered.
// an upper bound on the COMPUTED dist2 of every point in a box, the mirror image of oct_box_lb: per axis |q - p| <= max(q - lo, hi - q) for
// lo <= p <= hi, the rounded subtraction is monotone and antisymmetric, and squares and sums of non-negative terms are monotone
__device__ __forceinline__ double oct_box_ub(double qx, double qy, double qz, const float4 a, const float4 b) {
  const double g0 = fmax(__dsub_rn(qx, (double)a.x), __dsub_rn((double)a.w, qx));
  const double g1 = fmax(__dsub_rn(qy, (double)a.y), __dsub_rn((double)b.x, qy));
  const double g2 = fmax(__dsub_rn(qz, (double)a.z), __dsub_rn((double)b.y, qz));
  return __dadd_rn(__dadd_rn(__dmul_rn(g0, g0), __dmul_rn(g1, g1)), __dmul_rn(g2, g2));
}

template <class Offer, class Reset, class Stop, class Open, class Seed>
__device__ __forceinline__ void traverse(const GridView& g, const TreeView* tree, double qx, double qy, double qz, int seed_k, Offer&& offer, Reset&& reset,
                                         Stop&& stop, Open&& open, Seed&& seed) {
  auto scan_run = [&](unsigned int a, unsigned int b) {
    for (unsigned int j = a; j < b; ++j) {
      const PointRec* p = g.crec + j;
      offer(dist2(qx, qy, qz, p->x, p->y, p->z), p);
    }
  };
  const int cx = home_cell(qx, g.ox, g.inv_h, g.dx), cy = home_cell(qy, g.oy, g.inv_h, g.dy), cz = home_cell(qz, g.oz, g.inv_h, g.dz);
  int rprev = -1;   // the cells within this Chebyshev distance of (cx, cy, cz) are scanned
  for (int r = 1;; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.dy - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dz - 1);
    if (r > 1 && (long long)(x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1) > 2ll * g.n) {
      // far from everything in a sparse grid: the cloud itself is the smaller scan
      reset();
      scan_run(0u, (unsigned int)g.n);
      return;
    }
    for (int iz = z0; iz <= z1; ++iz)
      for (int iy = y0; iy <= y1; ++iy) {
        const bool inner = max(abs(iz - cz), abs(iy - cy)) <= rprev;   // a row the smaller block held: only its cells beyond that block
        for (int ix = x0; ix <= x1; ++ix) {
          if (inner && ix >= cx - rprev && ix <= cx + rprev) { ix = cx + rprev; continue; }
          const unsigned long long key = cell_key(ix, iy, iz);
          unsigned int slot = hash_slot(key, g.shift) & g.mask;
          HashEntry e = g.table[slot];
          while (e.key != key && e.key != kEmptyKey) { slot = (slot + 1) & g.mask; e = g.table[slot]; }
          if (e.key != kEmptyKey) scan_run(e.start, e.start + e.count);
        }
      }
    rprev = r;
    const double fx = g.ox + (cx - r) * g.h, fy = g.oy + (cy - r) * g.h, fz = g.oz + (cz - r) * g.h;
    const double w = (2 * r + 1) * g.h;
    double m = INFINITY;
    if (cx - r > 0) m = fmin(m, qx - fx);
    if (cx + r < g.dx - 1) m = fmin(m, fx + w - qx);
    if (cy - r > 0) m = fmin(m, qy - fy);
    if (cy + r < g.dy - 1) m = fmin(m, fy + w - qy);
    if (cz - r > 0) m = fmin(m, qz - fz);
    if (cz + r < g.dz - 1) m = fmin(m, fz + w - qz);
    if (m == INFINITY) return;   // the block covers the grid
    m *= 0.999;
    if (m > 0.0 && stop(m * m)) return;
    if (r == kTreeAfter && tree != nullptr) break;
  }
  reset();
  const TreeView t = *tree;
  if (seed_k > 0) {
    // The walk below visits the boxes in the tree's own order, so until the list is full it prunes nothing.  seed(ub) gives it a bound to
    // start with: a greedy descent (the child with the smallest lower bound) to the deepest node that still holds seed_k points; all of
    // them are at most ub = oct_box_ub of that node away, so the seed_k-th candidate is not beyond ub.
    long long width = 1;   // leaves under the node
    for (long long f = t.first_leaf; f > 0; f = (f - 1) >> 3) width <<= 3;
    long long id = 0, first = 0;   // the node and the first node of its level
    for (;;) {
      const long long lo = min((id - first) * width * t.leaf, (long long)g.n), hi = min(lo + width * t.leaf, (long long)g.n);
      if (hi - lo < seed_k) break;
      const float4* bx = reinterpret_cast<const float4*>(t.oct + 8 * (size_t)id);
      seed(oct_box_ub(qx, qy, qz, bx[0], bx[1]));
      if (id >= t.first_leaf) break;
      double best = INFINITY; long long pick = 8 * id + 1;
#pragma unroll 1   // (rare path: eight boxes in flight would cost the common path 35 VGPRs)
      for (int ch = 1; ch <= 8; ++ch) {
        const float4* cb = reinterpret_cast<const float4*>(t.oct + 8 * (size_t)(8 * id + ch));
        const double lb = oct_box_lb(qx, qy, qz, cb[0], cb[1]);
        if (lb < best) { best = lb; pick = 8 * id + ch; }
      }
      id = pick; first = 8 * first + 1; width >>= 3;
    }
  }
  long long id = 0;
  for (;;) {
    const float4* bx = reinterpret_cast<const float4*>(t.oct + 8 * (size_t)id);
    const double lb = oct_box_lb(qx, qy, qz, bx[0], bx[1]);
    if (lb < INFINITY && open(lb)) {   // (an empty leaf keeps an inverted box: lb = +inf)
      if (id < t.first_leaf) { id = 8 * id + 1; continue; }
      const long long j = id - t.first_leaf;
      const int lo = (int)min(j * t.leaf, (long long)g.n), hi = min(lo + t.leaf, g.n);
      for (int k = lo; k < hi; ++k) {
        const PointRec* p = t.srec + k;
        offer(dist2(qx, qy, qz, p->x, p->y, p->z), p);
      }
    }
    while (id != 0 && (id & 7) == 0) id = (id - 1) >> 3;   // the last of eight children: up
    if (id == 0) return;
    ++id;
  }
}
}  // namespace

}  // namespace mvicp
