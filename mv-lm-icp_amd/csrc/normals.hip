// f1 — Frame::recomputeNormals (src/internal/frame.cpp:244-255): for every point the k = 10 nearest points of its own
// cloud INCLUDING itself (Frame::getNeighbours, frame.cpp:208-231 -> nanoflann knnSearch), then pointSetPCA
// (include/common.h:331-346): centroid, covariance of the centred neighbours, eigenvector of the smallest eigenvalue,
// flipped so that n_z <= 0 (towards the camera).
//
// k-NN through the spatial hash built at upload: traverse() of knn_traverse.h without a box tree (its cell-order positions feed the PCA
// loops), keeping the k best (d2, cell-order position, original index) in LDS; the set is provably exact once the k-th distance is below
// the distance to the block's faces, and the block grows until that holds (r = 1 almost always: cells hold ~6 points).  Distances use the
// reference metric (include/frame.h:70-76, no fma).
// EXACT TIES.  The reference's clouds are range-image lattices (z quantised to 1 mm): 7 % of the Bunny points have a tie at the 10th
// place, and which of the tied points nanoflann returns is decided by the order in which its KD-tree visits them
// (KNNResultSet::addPoint keeps what came first, nanoflann.hpp:75-134; searchLevel visits the near child first, :1199-1247).  A
// "lowest index" rule picks a different neighbour set for 2-4 % of the points (normals up to 20 degrees apart, final Bunny poses 4.5e-5
// apart after 20 rounds).  So equal distances are ordered the way that tree would visit them: VisitTree below is the split structure
// nanoflann builds for this cloud (leaf size 1, frame.cpp:189), restated from the published algorithm, and two tied points are ordered by
// their lowest common ancestor — the child on the query's side of the split plane is visited first.  Result lists then equal
// knnSearch's element for element (order included: equal distances appear in visit order there too).
// The 3x3 symmetric eigenproblem is solved by the cyclic Jacobi rotations of jacobi3.h in fp64 (Eigen's SelfAdjointEigenSolver is an
// iterative QR on the same matrix: the eigenvector agrees to rounding, not bit for bit).
#include <algorithm>
#include <vector>

#include "common.h"
#include "jacobi3.h"
#include "kdvisit.h"
#include "knn_traverse.h"
#include "nn_metric.h"
#include "nn_tie.h"

namespace mvicp {

namespace {

constexpr int NT = 128;     // per-thread candidate lists live in LDS: KMAX x NT x 20 B = 40 KB per workgroup
constexpr int KMAX = 16;

struct NormJob {
  VisitTree tie;
  GridView g;
  const int* inv;    // original index -> sorted (canonical) position
  int k;
  double* nor_out;   // n x 3, original order
  double* snor_out;  // n x 3, sorted order (what the gather kernel reads)
  int* knn_out;      // n x k original indices (optional, for tests), ascending distance, equal distances in the tree's visit order
};

// the unit eigenvector of the smallest eigenvalue, flipped so that n_z <= 0: at most 12 sweeps, left as soon as the off-diagonal is gone
__device__ __forceinline__ void jacobi_min_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double* v) {
  jacobi3::M33 A = {a00, a01, a02, a01, a11, a12, a02, a12, a22}, V = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = fabs(A.m01) + fabs(A.m02) + fabs(A.m12);
    const double diag = fabs(A.m00) + fabs(A.m11) + fabs(A.m22);
    if (off <= 1e-18 * diag || off == 0.0) break;
    jacobi3::sweep(A, V);
  }
  const bool b1 = A.m11 < A.m00;
  const bool b2 = A.m22 < (b1 ? A.m11 : A.m00);
  double nx = b2 ? V.m02 : b1 ? V.m01 : V.m00, ny = b2 ? V.m12 : b1 ? V.m11 : V.m10, nz = b2 ? V.m22 : b1 ? V.m21 : V.m20;
  const double nn = sqrt(nx * nx + ny * ny + nz * nz);
  nx /= nn; ny /= nn; nz /= nn;
  if (nz > 0) { nx = -nx; ny = -ny; nz = -nz; }  // common.h:343 `if (normal(2) > 0) normal = -normal`
  v[0] = nx; v[1] = ny; v[2] = nz;
}

__global__ __launch_bounds__(NT) void normals_kernel(NormJob job) {
  const int i = blockIdx.x * NT + threadIdx.x;  // position in cell order
  if (i >= job.g.n) return;
  const PointRec me = job.g.crec[i];
  const int K = job.k;
  // the thread's current k best, ascending: distance, cell-order position, original index.  In LDS (one column per thread, no bank
  // conflicts) rather than in register arrays: the insertion below indexes them at run time, and this kernel runs once per cloud
  __shared__ double s_bd[KMAX][NT];
  __shared__ int s_bj[KMAX][NT];
  __shared__ long long s_bo[KMAX][NT];
#define bd(t) s_bd[t][threadIdx.x]
#define bj(t) s_bj[t][threadIdx.x]
#define bo(t) s_bo[t][threadIdx.x]
  auto reset = [&]() {
#pragma unroll
    for (int t = 0; t < KMAX; ++t) { bd(t) = 1.7976931348623157e308; bj(t) = -1; bo(t) = 0x7fffffffffffffffLL; }
  };
  // sorted insertion (ascending distance; equal distances in the tree's visit order): for a fixed query a strict total order, so the
  // list does not depend on the order of the offers.  One comparator call site, plain indexed arrays: this kernel runs once per cloud,
  // simplicity beats register residency here.
  auto offer = [&](double d, const PointRec* p) {
    const long long o = p->idx;
    int pos = K;
    while (pos > 0) {
      const double ed = bd(pos - 1);
      bool before = d < ed;
      if (!before && d == ed) before = bj(pos - 1) < 0 || visited_before(job.tie, me.x, me.y, me.z, o, bo(pos - 1));
      if (!before) break;
      --pos;
    }
    if (pos < K) {
      for (int t = K - 1; t > pos; --t) { bd(t) = bd(t - 1); bj(t) = bj(t - 1); bo(t) = bo(t - 1); }
      bd(pos) = d; bj(pos) = (int)(p - job.g.crec); bo(pos) = o;
    }
  };
  auto stop = [&](double m2) { return bj(K - 1) >= 0 && bd(K - 1) < m2; };   // the list is full and its K-th distance inside the block
  auto open = [](double) { return true; };
  auto seed = [](double) {};
  reset();
  traverse(job.g, nullptr, me.x, me.y, me.z, 0, offer, reset, stop, open, seed);
  // PCA of the neighbours (common.h:331-346).  Coordinates are taken relative to the point itself before the centroid is formed: the covariance is
  // the same, but a coordinate that all neighbours share (a range image's constant depth, an axis-aligned wall) then cancels EXACTLY — the mean of the
  // raw coordinates need not reproduce it (ten times 0.1 is not 1) and would leave a ~1e-17 residue that tilts the normal of an exact plane off the axis.
  double mx = 0, my = 0, mz = 0;
  int kk = 0;
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t < K && bj(t) >= 0) { const PointRec p = job.g.crec[bj(t)]; mx += p.x - me.x; my += p.y - me.y; mz += p.z - me.z; ++kk; }
  mx /= kk; my /= kk; mz /= kk;
  double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
#pragma unroll
  for (int t = 0; t < KMAX; ++t)
    if (t < K && bj(t) >= 0) {
      const PointRec p = job.g.crec[bj(t)];
      const double x = (p.x - me.x) - mx, y = (p.y - me.y) - my, z = (p.z - me.z) - mz;
      c00 += x * x; c01 += x * y; c02 += x * z; c11 += y * y; c12 += y * z; c22 += z * z;
    }
  double nv[3];
  jacobi_min_eigvec(c00, c01, c02, c11, c12, c22, nv);
  double* o = job.nor_out + 3 * (size_t)me.idx;
  o[0] = nv[0]; o[1] = nv[1]; o[2] = nv[2];
  double* os = job.snor_out + 3 * (size_t)job.inv[me.idx];
  os[0] = nv[0]; os[1] = nv[1]; os[2] = nv[2];
  if (job.knn_out) {
#pragma unroll
    for (int t = 0; t < KMAX; ++t)
      if (t < K) job.knn_out[(size_t)me.idx * K + t] = bj(t) >= 0 ? (int)bo(t) : -1;   // nanoflann's result order
  }
}

#undef bd
#undef bj
#undef bo

}  // namespace

int launch_normals(mvicp_ctx* c, FrameDev& f, int k, int* d_knn) {
  if (!f.has_grid) { set_error("normals need the per-cloud hash structure"); return MVICP_ERR_STATE; }
  if (k < 3 || k > KMAX) { set_error("k = %d outside [3, %d]", k, KMAX); return MVICP_ERR_ARG; }
  // tie order: nanoflann's tree for this cloud — built once per cloud upload and kept with the frame (nn_tie.hip; the 1-NN kernels'
  // tie rule uses the same tree), like the reference's own lazy index (frame.cpp:209-214)
  {
    int fi = -1;
    for (int t = 0; t < c->n_frames; ++t) if (&c->frames[t] == &f) fi = t;
    if (fi < 0) { set_error("normals: frame is not part of the context"); return MVICP_ERR_ARG; }
    MV_CHECK(ensure_tie_trees(c, std::vector<int>(1, fi)));
  }
  NormJob j;
  j.tie.nodes = static_cast<const VisitNode*>(f.tie_nodes); j.tie.slot = f.tie_slot;
  fill_grid_view(&j.g, f.grid, f.n);
  j.inv = f.grid.inv;
  j.k = k; j.nor_out = f.nor; j.snor_out = f.grid.snor; j.knn_out = d_knn;
  {
    ProfScope ps(c, "normals", 0.0);
    hipLaunchKernelGGL(normals_kernel, dim3((f.n + NT - 1) / NT), dim3(NT), 0, c->stream, j);
  }
  MV_HIP(hipGetLastError());
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
}

}  // namespace mvicp
