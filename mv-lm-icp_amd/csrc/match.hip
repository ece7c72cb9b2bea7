// Descriptor matching (mvicp_feature_match): for every row of A the two nearest rows of B, and for every row of B the two nearest rows
// of A, under the squared Euclidean distance in `dim` dimensions, as a pure function of the input bytes, bit for bit.  The contract is
// stated in include/mvicp.h; tests/matchref.py is its numpy form and its scalar-loop form.  DESIGN.md §3.11.
//
//   dist(a, b)   s = +0.0; for c = 0 .. dim-1 ascending: t = a[c] - b[c]; s = s + t * t      (fp64, every operation rounded on its own)
//
// Brute force, no search structure: one direction is one launch of the same kernel, the other the same launch with the operands swapped
// ((a - b) and (b - a) are exact negatives, so the distance is the same bits in both).
//   1  match_kernel<33>      a lane owns one row of the left operand in registers; a tile of 64 rows of the right operand is staged in LDS
//                            and every lane reads the same address (a broadcast: no bank conflicts); each lane keeps its best two (d2, j).
//                            The right operand is split over blockIdx.y into chunks, so that few left rows still fill the device.  The
//                            partial sums of non-negative terms only grow under rounded addition, so a candidate whose running sum
//                            already exceeds the lane's second best cannot enter: checked after each 11-bin sub-histogram, skipped
//                            only when the whole wave agrees.
//      match_generic_kernel  any 1 <= dim <= 64: 64 left rows per workgroup, transposed in LDS (lane-contiguous: no bank conflicts)
//   2  match_merge_kernel    per left row the best two over its chunks in (d2, j) order.  Tiling cannot change a pair's dist, and the
//                            chunks are visited in ascending j, so the merge is exact.
#include "common.h"
#include "match_tile.h"

namespace mvicp {

namespace {

using match_tile::Best2; using match_tile::RegTile; using match_tile::scan_reg; using match_tile::scan_generic; using match_tile::merge_row;

// the launch arithmetic below is written in these; the tile loops of match_tile.h in their namesakes
constexpr int kThreads = 256;   // left rows per workgroup of match_kernel
constexpr int kTile = 64;       // right rows per LDS tile
constexpr int kGenRows = 64;    // left rows per workgroup of match_generic_kernel
constexpr int kGenTile = 32;    // its right rows per LDS tile
constexpr int kMaxDim = 64;
constexpr int kMaxChunks = 65535;
static_assert(kThreads == match_tile::kThreads && kTile == match_tile::kTile && kGenRows == match_tile::kGenRows && kGenTile == match_tile::kGenTile &&
              kMaxDim == match_tile::kMaxDim, "the launches and the tile loops agree on the tiling");

template <int DIM>
__global__ __launch_bounds__(kThreads) void match_kernel(const double* __restrict__ A, int m, const double* __restrict__ B, int n, int chunk,
                                                         Best2* __restrict__ part) {
  __shared__ double Bs[kTile * RegTile<DIM>::LD];
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool live = i < m;
  const long long lo = (long long)blockIdx.y * chunk;
  const long long hi = lo + chunk < (long long)n ? lo + chunk : (long long)n;
  double d0 = INFINITY, d1 = INFINITY; int j0 = -1, j1 = -1;
  scan_reg<DIM>(A, i, live, B, lo, hi, Bs, d0, j0, d1, j1);
  if (live) { Best2* o = part + ((size_t)blockIdx.y * m + i); o->d0 = d0; o->d1 = d1; o->j0 = j0; o->j1 = j1; }
}

__global__ __launch_bounds__(kGenRows) void match_generic_kernel(const double* __restrict__ A, int m, const double* __restrict__ B, int n, int dim,
                                                                 int chunk, Best2* __restrict__ part) {
  __shared__ double As[kMaxDim * kGenRows];   // [c][row]
  __shared__ double Bs[kGenTile * kMaxDim];   // [row][c]
  const long long i0 = (long long)blockIdx.x * kGenRows;
  const long long i = i0 + threadIdx.x;
  const bool live = i < m;
  const long long lo = (long long)blockIdx.y * chunk;
  const long long hi = lo + chunk < (long long)n ? lo + chunk : (long long)n;
  double d0 = INFINITY, d1 = INFINITY; int j0 = -1, j1 = -1;
  scan_generic(A, m, i0, B, lo, hi, dim, As, Bs, d0, j0, d1, j1);
  if (live) { Best2* o = part + ((size_t)blockIdx.y * m + i); o->d0 = d0; o->d1 = d1; o->j0 = j0; o->j1 = j1; }
}

// rows x 2 results from the rows x chunks partial lists (chunks == 0: the padding alone)
__global__ __launch_bounds__(kThreads) void match_merge_kernel(const Best2* __restrict__ part, int rows, int chunks, int* __restrict__ idx,
                                                               double* __restrict__ d2) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows) return;
  double d0 = INFINITY, d1 = INFINITY; int j0 = -1, j1 = -1;
  merge_row(part, (size_t)rows, (size_t)i, chunks, d0, j0, d1, j1);
  idx[2 * i] = j0; idx[2 * i + 1] = j1;
  d2[2 * i] = d0; d2[2 * i + 1] = d1;
}

__global__ __launch_bounds__(kThreads) void match_finite_kernel(const double* __restrict__ v, size_t count, int* __restrict__ flag) {
  bool bad = false;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < count; e += (size_t)gridDim.x * kThreads) bad |= !isfinite(v[e]);
  if (bad) atomicOr(flag, 1);
}

// rows of the right operand per chunk and the number of chunks for `right` rows
void chunking(const mvicp_ctx* c, long long right, int* chunk, int* chunks) {
  long long ch = c->match_chunk > 0 ? c->match_chunk : 1;
  if ((right + ch - 1) / ch > kMaxChunks) ch = (right + kMaxChunks - 1) / kMaxChunks;
  if (ch > right) ch = right > 0 ? right : 1;
  *chunk = (int)ch;
  *chunks = (int)((right + ch - 1) / ch);
}

int launch_direction(mvicp_ctx* c, const char* scope, const double* L, int rows, const double* Rt, int right, int dim, int chunk, int chunks, Best2* part) {
  // the left rows once, the right rows once per workgroup of left rows, the partial lists
  const double wgs = dim == 33 ? (rows + kThreads - 1) / kThreads : (rows + kGenRows - 1) / kGenRows;
  ProfScope ps(c, scope, 8.0 * dim * ((double)rows * chunks + wgs * right) + sizeof(Best2) * (double)rows * chunks);
  if (dim == 33) {
    const dim3 grid((unsigned int)((rows + kThreads - 1) / kThreads), (unsigned int)chunks);
    hipLaunchKernelGGL(match_kernel<33>, grid, dim3(kThreads), 0, c->stream, L, rows, Rt, right, chunk, part);
  } else {
    const dim3 grid((unsigned int)((rows + kGenRows - 1) / kGenRows), (unsigned int)chunks);
    hipLaunchKernelGGL(match_generic_kernel, grid, dim3(kGenRows), 0, c->stream, L, rows, Rt, right, dim, chunk, part);
  }
  MV_HIP(hipGetLastError());
  return MVICP_OK;
}

}  // namespace

long long feature_match(mvicp_ctx* c, const double* A, int a_on_device, long long m, const double* B, int b_on_device, long long n, int dim) {
  c->match.m = -1; c->match.n = -1;   // (the last result ends here; a failed call leaves none behind)
  hipStream_t st = c->stream;
  const size_t M = (size_t)m, N = (size_t)n, a_bytes = 8 * M * dim, b_bytes = 8 * N * dim;
  int chunk_f = 1, chunks_f = 0, chunk_b = 1, chunks_b = 0;
  if (m > 0 && n > 0) { chunking(c, n, &chunk_f, &chunks_f); chunking(c, m, &chunk_b, &chunks_b); }
  // results: [fwd_idx | fwd_d2 | bwd_idx | bwd_d2 | flag]
  const size_t off_fd = align256(8 * M), off_bi = off_fd + align256(16 * M), off_bd = off_bi + align256(8 * N), off_flag = off_bd + align256(16 * N);
  MV_CHECK(c->match.dev.reserve(off_flag + 256));
  // scratch: [A staged | B staged | forward partial lists | backward partial lists]
  const size_t off_b = a_on_device ? 0 : align256(a_bytes), off_pf = off_b + (b_on_device ? 0 : align256(b_bytes));
  const size_t off_pb = off_pf + align256(sizeof(Best2) * M * chunks_f), tmp_need = off_pb + align256(sizeof(Best2) * N * chunks_b);
  MV_CHECK(c->match.tmp.reserve(tmp_need + 256));
  c->match.fwd_idx = reinterpret_cast<int*>(c->match.dev.p); c->match.fwd_d2 = reinterpret_cast<double*>(c->match.dev.p + off_fd);
  c->match.bwd_idx = reinterpret_cast<int*>(c->match.dev.p + off_bi); c->match.bwd_d2 = reinterpret_cast<double*>(c->match.dev.p + off_bd);
  int* flag = reinterpret_cast<int*>(c->match.dev.p + off_flag);
  const double* dA = A; const double* dB = B;
  if (!a_on_device && a_bytes) { MV_HIP(hipMemcpyAsync(c->match.tmp.p, A, a_bytes, hipMemcpyHostToDevice, st)); dA = reinterpret_cast<const double*>(c->match.tmp.p); }
  if (!b_on_device && b_bytes) { MV_HIP(hipMemcpyAsync(c->match.tmp.p + off_b, B, b_bytes, hipMemcpyHostToDevice, st)); dB = reinterpret_cast<const double*>(c->match.tmp.p + off_b); }
  MV_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  const double* checked[2] = {dA, dB};
  const size_t counts[2] = {M * dim, N * dim};
  for (int t = 0; t < 2; ++t)
    if (counts[t]) {
      const size_t wgs = (counts[t] + kThreads - 1) / kThreads;
      hipLaunchKernelGGL(match_finite_kernel, dim3((unsigned int)(wgs < 4096 ? wgs : 4096)), dim3(kThreads), 0, st, checked[t], counts[t], flag);
      MV_HIP(hipGetLastError());
    }
  int h_flag = 0;
  MV_HIP(hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  MV_HIP(hipStreamSynchronize(st));
  if (h_flag) { set_error("a descriptor value is not finite"); return MVICP_ERR_ARG; }
  Best2* part_f = reinterpret_cast<Best2*>(c->match.tmp.p + off_pf);
  Best2* part_b = reinterpret_cast<Best2*>(c->match.tmp.p + off_pb);
  if (chunks_f) {
    MV_CHECK(launch_direction(c, "match_fwd", dA, (int)m, dB, (int)n, dim, chunk_f, chunks_f, part_f));
    MV_CHECK(launch_direction(c, "match_bwd", dB, (int)n, dA, (int)m, dim, chunk_b, chunks_b, part_b));
  }
  {
    ProfScope ps(c, "match_merge", (sizeof(Best2) * (double)chunks_f + 24.0) * m + (sizeof(Best2) * (double)chunks_b + 24.0) * n);
    if (m) hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned int)((M + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part_f, (int)m, chunks_f, c->match.fwd_idx, c->match.fwd_d2);
    if (n) hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned int)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part_b, (int)n, chunks_b, c->match.bwd_idx, c->match.bwd_d2);
    MV_HIP(hipGetLastError());
  }
  MV_HIP(hipStreamSynchronize(st));
  c->match.m = m; c->match.n = n;
  return m;
}

}  // namespace mvicp
