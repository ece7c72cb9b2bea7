/* mvicp.h — C ABI of libmvicp_hip.so: the MI355X (gfx950) multiview LM-ICP hot path.
 *
 * This is the drop-in boundary.  The reference (adrelino/mv-lm-icp) has no FFI: its
 * seams are plain C++ members/free functions.  Each entry point below names the reference interface
 * it replaces (file:line relative to the reference tree).  Plain pointers and sizes only; every call
 * returns 0 on success or a negative mvicp_status (one exception, stated at its declaration: mvicp_get_correspondences
 * returns the number of triples it wrote, >= 0), and mvicp_last_error() holds the message.  Test `< 0` for failure.  The
 * library owns all device memory; the caller owns every host buffer it passes.  One context drives
 * one GPU (one process per GPU; see mvicp_set_shard / mvicp_comm_init for the multi-GPU path).
 *
 * A REFUSED CALL CHANGES NOTHING.  An entry point that returns MVICP_ERR_ARG or MVICP_ERR_STATE for its arguments or the call order has
 * decided so before it touched the context: clouds, structures, pending builds, the graph, lists, epochs, normals and options are what they
 * were, and every later call computes what it would have computed without the refused one (tests/test_gpu_rejected_calls.py).  Only the
 * error string, profile counters and performance-only state (a queued evaluation, the validity of a cache) may differ.  Each set-up entry
 * below says what a non-OK return leaves; the exceptions are stated where they apply (mvicp_correspond: any non-OK return drops the
 * cross-round state, see mvicp_correspondence_epochs; errors that are found on the device after work has begun).
 *
 * Conventions
 *   pose    : 16 doubles, 4x4 COLUMN-major = Eigen::Isometry3d::data()  (include/frame.h:42)
 *   points  : n x 3 doubles AoS = &std::vector<Eigen::Vector3d>[0]      (include/frame.h:38-39)
 *   edge e  : directed src -> dst = Frame::neighbours[j] of frame src    (include/frame.h:24-29,46)
 *   indices : int32, local to their frame
 */
#ifndef MVICP_H
#define MVICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvicp_ctx mvicp_ctx;

enum mvicp_status {
  MVICP_OK = 0,
  MVICP_ERR_ARG = -1,      /* bad argument / call order */
  MVICP_ERR_HIP = -2,      /* HIP runtime error (no GPU, OOM, launch failure) */
  MVICP_ERR_STATE = -3,    /* frames/graph/correspondences not set */
  MVICP_ERR_COMM = -4,     /* RCCL failure */
  MVICP_ERR_NUMERIC = -5,  /* LM solve failed (non-finite / not positive definite) */
  MVICP_ERR_INTERNAL = -6  /* a host-side C++ exception (out of memory, thread creation, ...) was caught at the boundary */
};

/* Rotation parameterization of the LM solve = which reference optimizer is mirrored. */
enum mvicp_param {
  MVICP_PARAM_EIGEN_QUATERNION = 0, /* ICP_Ceres::ceresOptimizer            src/internal/icp-ceres.cpp:220-323 */
  MVICP_PARAM_ANGLE_AXIS = 1,       /* ICP_Ceres::ceresOptimizer_ceresAngleAxis              :325-395 */
  MVICP_PARAM_SOPHUS_SE3 = 2        /* ICP_Ceres::ceresOptimizer_sophusSE3                   :398-475 */
};

/* Nearest-neighbour kernels (all exact; identical results by construction). */
enum mvicp_nn_method {
  MVICP_NN_AUTO = 0,
  MVICP_NN_BRUTE = 1, /* LDS-tiled exhaustive scan */
  MVICP_NN_GRID = 2,  /* per-query: spatial-hash (uniform grid) lookup with exact AABB-tree fallback */
  MVICP_NN_TILE = 3   /* per-wave: 64 curve-adjacent queries share a pruned brute force over LDS-staged 32-point tiles */
};

const char* mvicp_last_error(void);
/* "name major.minor" of the build, and the gfx arch the kernels were compiled for. */
const char* mvicp_version(void);

/* ---- lifetime -------------------------------------------------------------------------------- */
int mvicp_create(int device, mvicp_ctx** out);
int mvicp_destroy(mvicp_ctx* ctx);

/* ---- data upload (once; clouds are static in their local frame) ------------------------------- */
/* Replaces Frame::pts / Frame::nor as the kernel-visible copy (include/frame.h:38-39) and the lazy
 * KD-tree build of Frame::getClosestPoint (src/internal/frame.cpp:188-193): the per-cloud NN
 * structure is built here, once.  nrm may be NULL (point-to-point only).  The call returns when the cloud is on the device; the
 * structures themselves (k-d order, box hierarchy, matrix-pipe operands, hash) are built behind it on a host thread from a private copy
 * of the cloud, so that the clouds of an upload loop are built side by side (option "async_build", default 1); the first entry point that
 * needs a structure (mvicp_set_graph, mvicp_nn_query, mvicp_recompute_normals) waits for the pending builds and reports a failed one. */
/* Non-OK returns.  mvicp_set_num_frames: n_frames < 0 -> MVICP_ERR_ARG, and the frames, the graph and every stage's last result stay.
 * mvicp_set_frame: a frame index out of range, n < 0, xyz NULL with n > 0, a non-finite coordinate -> MVICP_ERR_ARG; called while a graph
 * exists -> MVICP_ERR_STATE.  All of these are decided before the frame is touched (the coordinates are scanned first): the frame keeps
 * the cloud it held, with its structures, its pending build and its answers, or stays empty if it was empty.  MVICP_ERR_HIP (an
 * allocation or a copy failed after the old cloud was released) leaves the frame EMPTY (n = 0), never holding undefined bytes.  With
 * "async_build" 0 a failed build is returned by this call and is sticky like a failed background build: the frame is unusable and says
 * why until it is uploaded again. */
int mvicp_set_num_frames(mvicp_ctx* ctx, int n_frames);
int mvicp_set_frame(mvicp_ctx* ctx, int frame, const double* xyz, const double* nrm, int n);

/* The same upload from DEVICE memory: a cloud that already lives in HBM (a torch tensor of a GPU pre-processing step, a depth-fusion
 * result) is built into the same structures without a trip through host memory.  d_xyz / d_nrm: n x 3 row-major doubles in device memory
 * of the context's device (d_nrm may be NULL); a host pointer or another device's pointer is MVICP_ERR_ARG.  The arrays must be fully
 * written when the call is made (the caller synchronises the stream that produced them); the call copies them device-to-device into
 * library-owned buffers before it returns, so the caller may free or overwrite them afterwards.  Everything else is mvicp_set_frame's:
 * before mvicp_set_graph, a non-finite coordinate is MVICP_ERR_ARG reported by this call, option "async_build" moves the rest of the
 * build behind the call (a failed build is reported, sticky, by the next entry point that needs the structures).  The structures are
 * built on the GPU and are byte-identical to the ones mvicp_set_frame builds on the host for the same cloud and options.
 * Non-OK returns: as mvicp_set_frame's.  The finiteness / bounds reduction runs over the CALLER's array before the frame is touched, so
 * MVICP_ERR_ARG (index, n, a NULL / host / foreign pointer, a non-finite coordinate) and MVICP_ERR_STATE (a graph exists) leave the frame
 * exactly as it was; MVICP_ERR_HIP after the old cloud was released leaves it empty. */
int mvicp_set_frame_device(mvicp_ctx* ctx, int frame, const double* d_xyz, const double* d_nrm, int n);

/* Read-back seam of the per-cloud structures (tests, diagnosis).  Waits for pending builds, then copies the named array of `frame` into
 * out (host memory, cap_bytes long) or, with out NULL, only reports its size.  RETURNS THE BYTE COUNT (>= 0) or a negative mvicp_status.
 * Names: "spts" "sidx" "srec" "crec" "inv" "snor" "table" "oct" "wide" "mf_ops" "mf_blk" "bricks" "celltab" (device arrays; absent
 * ones are 0 bytes), "h_order" "h_inv" (the host copies of the order), "scalars" and "build_ms".
 * "scalars" is one fp64 vector in this fixed order: dims[3], origin[3], cell, inv_cell, n_cells, table_mask, table_shift, oct_leaf,
 * oct_first_leaf, wide_levels, wide_cnt[6], wide_off[6], maxabs, struct_bytes, max_norm, bdims[3] (32 values).
 * "build_ms" is two doubles of the slot's last build: host wall milliseconds without the upload, device milliseconds of the device
 * build's kernels (-1 for a host build). */
long long mvicp_get_structure(mvicp_ctx* ctx, int frame, const char* name, void* out, long long cap_bytes);

/* Replaces Frame::recomputeNormals() (include/frame.h:49, src/internal/frame.cpp:244-255; on by default in the reference,
 * main_multiview.cpp:49,68-70): normal of every point = eigenvector of the smallest eigenvalue of the covariance of its
 * k nearest points INCLUDING itself (reference k = 10), flipped so n_z <= 0 (include/common.h:331-346).  Overwrites the
 * frame's device normals; nrm_out (n x 3) and knn_out (n x k original indices, nearest first) may be NULL.  May be called
 * at any time: correspondence lists that point into this frame are re-gathered with the new normals (the reference reads
 * dstCloud.nor when it builds the problem, icp-ceres.cpp:270-292).
 * Non-OK returns: a frame index out of range, k outside [3, 16] -> MVICP_ERR_ARG; fewer than k points, a frame without structures (empty,
 * or its build failed) -> MVICP_ERR_STATE.  All are decided before anything is allocated: the frame's normals are what they were, and a
 * frame uploaded WITHOUT normals still has none (point-to-plane evaluation keeps refusing it).  If the launch itself fails, the buffers
 * this call allocated for such a frame are released again; the normals of a frame that had some are then undefined until the next
 * successful call. */
int mvicp_recompute_normals(mvicp_ctx* ctx, int frame, int k, double* nrm_out, int* knn_out);

/* Pose graph = all Frame::neighbours[j].neighbourIdx (frame.cpp:67-89 builds it; main_multiview.cpp:
 * 104-117).  Edge order is the reference's loop order: src ascending, then neighbour order.
 * Non-OK returns: n_edges < 0, NULL lists with n_edges > 0, a frame index out of range, a self edge -> MVICP_ERR_ARG; a failed structure
 * build -> MVICP_ERR_STATE.  All are decided before the previous graph is released: it, its lists and its epochs keep working.  A failure
 * after that point (MVICP_ERR_HIP: an allocation) leaves a context whose graph must be set again. */
int mvicp_set_graph(mvicp_ctx* ctx, int n_edges, const int* src, const int* dst);

/* ---- overlap census and the pose graph made from it ----------------------------------------------------
 * The reference offers one rule for the pose graph: the k frames whose camera centres are nearest (Frame::computePoseNeighboursKnn,
 * frame.cpp:67-89; main_multiview.cpp:104-117).  mvicp_overlap measures instead how much surface two clouds share at the given poses,
 * for ALL ordered frame pairs at once.  For i != j:
 *   hits[i*K+j] = #{ p in S_i : sqrt(d2(p)) < (double)thresh }   -- the predicate of frame.cpp:156
 *   sumq[i*K+j] = sum over those p of floor(d2(p) * 2^q_exp)      -- exact integers, order-independent
 * d2(p) = squared distance, in the reference metric (frame.h:70-76, no fma), from the query R_j^-1 ((R_i p + t_i) - t_j) -- the SAME
 * rounded operations as mvicp_correspond's query transform -- to the nearest point of cloud j.  hits[i*K+i] = samples[i], sumq[i*K+i] = 0.
 * S_i: s_i = n_i if max_samples <= 0 or max_samples >= n_i, else max_samples; its t-th member is the point with ORIGINAL index
 * floor(t * n_i / s_i) (64-bit), t = 0 .. s_i-1.  samples[i] = s_i.
 * q_exp: the integer with 2^30 <= B2 * 2^q_exp < 2^31, B2 = the smallest double whose correctly rounded sqrt is >= thresh
 * (sqrt(d2) < thresh <=> d2 < B2), so every term is < 2^31 and exact.  A frame with n_i = 0 has samples[i] = 0 and zero hits in its row
 * and its column.
 *   poses : n_frames x 16;  samples: K ints;  hits: K*K ints;  sumq: K*K long long (may be NULL);  q_exp: one int (may be NULL).
 * Needs every frame uploaded (mvicp_set_frame / mvicp_set_frame_device; waits for pending structure builds and reports a failed one like
 * mvicp_nn_query) and NO graph: it may be called before or after mvicp_set_graph and between rounds, and it is HISTORY-NEUTRAL — it reads
 * clouds and structures only and leaves the temporal cache, seeds, lists, epochs, medians, the AUTO state and any queued evaluation
 * alone, so a registration with census calls in between is bit-identical to one without.  With several ranks every rank computes the
 * whole census locally (the clouds are replicated): identical arrays, no communication.
 * Errors: thresh not finite or <= 0, a non-finite pose entry, NULL poses / samples / hits -> MVICP_ERR_ARG; mvicp_set_num_frames not
 * called or a frame never uploaded -> MVICP_ERR_STATE. */
int mvicp_overlap(mvicp_ctx* ctx, const double* poses, float thresh, int max_samples, int* samples, int* hits, long long* sumq, int* q_exp);

/* ---- voxel-grid reduction: downsampled levels and the fused model -------------------------------------------
 * Reduces the points of one or several frames, at given poses, to ONE POINT PER OCCUPIED VOXEL: a coarser copy of a cloud (one frame, no
 * poses) or the merged model of a registration (all frames at the final poses).  The result is a pure function of the inputs, bit for bit
 * (tests/voxelref.py is the same definition in numpy):
 *   Inputs   frames[]: n_sel DISTINCT frame indices (NULL = all frames 0 .. K-1, n_sel ignored); poses: n_frames x 16 or NULL; voxel: the cell edge.
 *   Sequence the selected frames in the order of frames[], inside a frame the points in ascending ORIGINAL index; the position in it is `seq`.
 *   World    poses == NULL: w = p, m = n (the stored bytes, no arithmetic).  Otherwise, for c = 0..2, every operation rounded on its own, no fma
 *            (the first line of xf_point, csrc/nn_metric.h):  w_c = ((R[c,0] p0 + R[c,1] p1) + R[c,2] p2) + t_c,
 *            m_c = (R[c,0] n0 + R[c,1] n1) + R[c,2] n2.  R and t are used as given; they are not orthonormalised.
 *   Cell     c_a = floor(w_a / voxel) per axis, the IEEE double division (NOT a multiplication by 1 / voxel: that lands in another cell for
 *            points on cell faces).  Any |w_a / voxel| >= 2^31, or a non-finite quotient, is MVICP_ERR_ARG.
 *   Key      cmin_a and d_a = cmax_a - cmin_a + 1 over the whole sequence; key = ((c_z - cmin_z) d_y + (c_y - cmin_y)) d_x + (c_x - cmin_x);
 *            d_x d_y d_z >= 2^62 is MVICP_ERR_ARG (voxel too small for the extent).
 *   Output   one row per distinct key, rows in ASCENDING key (z-major, then y, then x).  Row v:
 *            cnt[v] (int32) = number of input points with that key;
 *            xyz[v]: per component s = +0.0; for the voxel's points in ascending seq: s = s + w_c; then s / (double)cnt (IEEE division);
 *            nrm[v]: the same sequential sums S of m, then S / sqrt((S0 S0 + S1 S1) + S2 S2) (no fma, IEEE sqrt and division), (0,0,0) when that
 *            norm is 0 or not finite; produced iff every selected frame with at least one point has normals (*has_normals).
 *   Empty    an empty selection, or one whose frames are all empty, gives m = 0 (*has_normals = 1) and is not an error.
 * The summation order is part of the contract, so a voxel is summed by one GPU lane: a voxel that holds thousands of points (a cell larger
 * than the cloud) is reduced sequentially -- correct, not fast.
 * Needs the selected frames uploaded (mvicp_set_frame / mvicp_set_frame_device), NO graph and no search structure; HISTORY-NEUTRAL like
 * mvicp_overlap: it reads the stored clouds only and leaves caches, seeds, lists, epochs, medians, the AUTO state and queued evaluations
 * alone.  With several ranks every rank computes it locally.  The call returns when the result is complete; the result lives in
 * library-owned device memory until the next mvicp_voxel_grid, mvicp_set_num_frames or mvicp_destroy.
 * RETURNS THE NUMBER OF VOXELS m (>= 0) or a negative mvicp_status; has_normals may be NULL.
 * Errors: NULL context, voxel not finite or <= 0, n_sel < 0, a non-finite pose entry, a frame index out of range or listed twice, the range
 * errors above, >= 2^31 input points -> MVICP_ERR_ARG (those that need no GPU are decided before the context is touched);
 * mvicp_set_num_frames not called or a selected frame never uploaded -> MVICP_ERR_STATE. */
long long mvicp_voxel_grid(mvicp_ctx* ctx, int n_sel, const int* frames, const double* poses, double voxel, int* has_normals);
/* Copies the last result: xyz / nrm (m x 3 doubles), cnt (m ints); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the
 * context's device (decided per pointer like mvicp_set_frame_device decides; another device's memory is MVICP_ERR_ARG), so a device
 * result goes straight back into mvicp_set_frame_device of this or another context.  cap = rows each destination holds.
 * Errors: cap < m -> MVICP_ERR_ARG; no mvicp_voxel_grid before, or nrm != NULL when has_normals == 0 -> MVICP_ERR_STATE. */
int mvicp_voxel_fetch(mvicp_ctx* ctx, long long cap, double* xyz, double* nrm, int* cnt);

/* ---- outlier removal: the statistical and the radius rule over one k-distance search ----------------------------
 * Cleans one cloud the way every point-cloud toolkit does: a point goes when its k nearest neighbours are unusually far away.  The result is
 * a pure function of the stored cloud p_0 .. p_{n-1} of `frame` (the stored bytes, no pose), bit for bit (tests/outlierref.py is the same
 * definition in numpy):
 *   Per point  D_i[0..k] = the k+1 smallest VALUES, ascending, of the multiset { dist2(p_i, p_j) : j = 0 .. n-1 }, j = i included (D_i[0] = +0);
 *              dist2 = (d0 d0 + d1 d1) + d2 d2, every operation rounded on its own, no fma (csrc/nn_metric.h).  Only the values enter: which
 *              of several equidistant points is "the" neighbour is irrelevant, so no tie order is needed or built.
 *              kd2_i = D_i[k];  mdist_i: s = +0.0; for t = 1 .. k: s = s + sqrt(D_i[t]) (IEEE sqrt, ascending t); then s / (double)k.
 *   Radius     on iff radius > 0: keep i iff sqrt(kd2_i) < radius (IEEE sqrt) -- at least k other points within the radius.
 *   Statistic  on iff std_ratio >= 0; order-independent by the device of the census's sumq.  mmax = max_i mdist_i.  mmax == 0: every point
 *              passes and q_exp = s1 = s2 = T = threshold = 0 (the same zeros are reported while the rule is off).  Otherwise q_exp = the integer
 *              with 2^30 <= mmax 2^q_exp < 2^31, M_i = floor(mdist_i 2^q_exp) (an exact scaling), S1 = sum M_i, S2 = sum M_i^2 (exact integers;
 *              S2 = s2_hi 2^64 + s2_lo), T = mvicp_outlier_threshold(n, S1, S2, std_ratio), and i passes iff (double)M_i <= T.
 *   Both on    kept iff it passes both;  both off: every point is kept (the call is then a k-distance query).
 *   Output     kept rows in ascending original index: xyz / nrm = the stored bytes (nrm iff the frame has normals), idx = the int32 original
 *              index; mdist and kd2 have length n, for ALL points.
 * Needs 1 <= k <= 32 and n > k (n = 0: zero rows, no error); needs the frame's hash structure (waits for pending builds and reports a failed
 * one, like mvicp_overlap), NO graph, and is HISTORY-NEUTRAL: it does not modify the frame and leaves caches, seeds, lists, epochs, medians, the
 * AUTO state and queued evaluations alone, so a registration with filter calls in between is bit-identical to one without.  With several
 * ranks every rank computes it locally.  The call returns when the result is complete; the result lives in library-owned device memory until
 * the next mvicp_outlier_filter, mvicp_set_num_frames or mvicp_destroy.  Profile scopes: "outlier_knn", "outlier_sum", "outlier_flag",
 * "outlier_compact".
 * RETURNS THE NUMBER KEPT (>= 0) or a negative mvicp_status; stats may be NULL.
 * Errors: NULL context, k outside [1, 32], a non-finite std_ratio or radius, a frame index out of range, 0 < n <= k, a neighbour distance that
 * overflows -> MVICP_ERR_ARG (those that need no GPU are decided before the context is touched); a frame never uploaded -> MVICP_ERR_STATE. */
typedef struct mvicp_outlier_stats {
  long long n, kept;
  int q_exp;
  int has_normals;   /* the frame had stored normals at this call: mvicp_outlier_fetch gives nrm (the filter selects in the same call) */
  unsigned long long s1, s2_hi, s2_lo;
  double T;          /* the threshold in quantised units (compared with (double)M_i) */
  double threshold;  /* ldexp(T, -q_exp): the same in the cloud's length unit */
} mvicp_outlier_stats;
long long mvicp_outlier_filter(mvicp_ctx* ctx, int frame, int k, double std_ratio, double radius, mvicp_outlier_stats* stats);
/* Copies the last result: xyz / nrm (kept x 3 doubles), idx (kept ints), mdist / kd2 (n doubles); each may be NULL; each may be a HOST pointer
 * or a DEVICE pointer of the context's device, decided per pointer as mvicp_voxel_fetch decides, so a device result goes straight into
 * mvicp_set_frame_device.  cap_kept = rows xyz / nrm / idx hold, cap_n = entries mdist / kd2 hold (looked at only when one of the two is given).
 * Errors: cap_kept < kept, cap_n < n -> MVICP_ERR_ARG; no mvicp_outlier_filter before, or nrm != NULL for a frame without normals -> MVICP_ERR_STATE. */
int mvicp_outlier_fetch(mvicp_ctx* ctx, long long cap_kept, double* xyz, double* nrm, int* idx, long long cap_n, double* mdist, double* kd2);
/* The threshold of the statistical rule (pure host function, no context): S2 = s2_hi 2^64 + s2_lo;
 *   mean = (double)S1 / (double)n;  var = ((double)(n S2 - S1^2) / (double)n) / ((double)n - 1.0);  *T = mean + std_ratio sqrt(var)
 * -- the 128-bit integer n S2 - S1^2 (>= 0) converted with round-to-nearest-even, every floating-point operation rounded on its own.
 * Errors: n < 2, NULL T, a non-finite std_ratio, n S2 >= 2^128 or S1^2 > n S2 -> MVICP_ERR_ARG. */
int mvicp_outlier_threshold(long long n, unsigned long long s1, unsigned long long s2_hi, unsigned long long s2_lo, double std_ratio, double* T);

/* ---- clusters: DBSCAN / Euclidean cluster extraction over one stored cloud; drop small clusters -------------------------
 * Answers "which points belong together", which the two outlier rules cannot: they judge the density of a k-neighbourhood and keep a compact
 * clump of stray points (a clamp, a hand, a piece of the turntable).  The result is a pure function of the stored cloud p_0 .. p_{n-1} of
 * `frame` (the stored bytes, no pose), bit for bit, whatever order the GPU's threads run in (tests/clusterref.py is the same definition in
 * numpy and as a scalar loop); only comparisons and integers enter:
 *   Adjacency  j in N(i) iff sqrt(dist2(p_i, p_j)) < radius (IEEE sqrt, strict) -- the predicate of mvicp_knn_search and
 *              mvicp_outlier_filter; equivalently dist2 < B2, B2 as defined at mvicp_overlap; dist2 = (d0 d0 + d1 d1) + d2 d2, every
 *              operation rounded on its own, no fma (csrc/nn_metric.h).  i in N(i) (d2 = +0).  dist2 is BITWISE SYMMETRIC in its arguments
 *              (the two differences are exact negatives of each other and the squares drop the sign), so the graph is undirected.
 *   Core       i is a core point iff |N(i)| >= min_pts; the point itself counts (as in sklearn and Open3D).  Only the comparison enters; no
 *              per-point count is output.
 *   Cluster    a connected component of the graph on the CORE points whose edges are {i, j}, both core, j in N(i).
 *   Border     a non-core i with at least one core point in N(i) joins the cluster of THE core point of N(i) that comes first in the order
 *              (dist2 ascending, original index ascending) -- the order of mvicp_knn_search; a minimum over a strict total order, so it
 *              does not depend on any visiting order.  A border point never links two clusters.
 *   Noise      every other point: label -1.
 *   Labels     the clusters are numbered 0 .. C-1 in ascending order of their smallest CORE original index (on core points this is sklearn's
 *              numbering).
 *   Output     label (n int32), core (n bytes, 1 = core), size (C int32, border members included), and the stats below; largest_label is the
 *              lowest label among the clusters of the largest size (-1 when C = 0).
 *   Limits     n = 0 gives zero clusters and is no error.  min_pts = 1 is plain Euclidean cluster extraction: every point is core, no noise.
 * Needs a finite radius > 0 and 1 <= min_pts <= 2^30; needs the frame's hash structure (waits for pending builds and reports a failed one,
 * like mvicp_overlap), NO graph, and is HISTORY-NEUTRAL: it does not modify the frame and leaves caches, seeds, lists, epochs, medians, the AUTO
 * state and queued evaluations alone, so a registration with cluster calls in between is bit-identical to one without.  With several ranks
 * every rank computes it locally.  The call returns when the result is complete; the result lives in library-owned device memory until the
 * next mvicp_cluster, an upload to `frame`, mvicp_set_num_frames or mvicp_destroy.  Profile scopes: "cluster_core", "cluster_union",
 * "cluster_border", "cluster_label", "cluster_compact".
 * RETURNS THE NUMBER OF CLUSTERS C (>= 0) or a negative mvicp_status; stats may be NULL.
 * Errors: NULL context, min_pts outside [1, 2^30], a radius that is not finite or <= 0, a frame index out of range -> MVICP_ERR_ARG, decided
 * before the context is touched: the previous result stays; a frame never uploaded -> MVICP_ERR_STATE; a neighbour distance that can
 * overflow -- with a = the largest |coordinate| of the cloud and t = a + a, (t t + t t) + t t = +inf, a bound on every dist2 of the cloud
 * -- -> MVICP_ERR_ARG, reported by this call, and no result is left behind. */
typedef struct mvicp_cluster_stats {
  long long n, clusters, core, border, noise;   /* core + border + noise = n */
  long long largest;                            /* size of the largest cluster (0 when there is none) */
  int largest_label;
  int has_normals;                              /* the frame had stored normals at this call.  What mvicp_cluster_fetch_kept gives is decided when
                                                   mvicp_cluster_select runs: nrm iff the frame has stored normals THEN (an adopt in between counts) */
} mvicp_cluster_stats;
long long mvicp_cluster(mvicp_ctx* ctx, int frame, double radius, int min_pts, mvicp_cluster_stats* stats);
/* Copies the last result: label (n ints), core (n bytes), size (C ints); each may be NULL; each may be a HOST pointer or a DEVICE pointer of
 * the context's device, decided per pointer as mvicp_voxel_fetch decides.  cap_n = entries label / core hold, cap_clusters = entries size holds
 * (each looked at only when one of its arrays is given).
 * Errors: NULL context, cap_n < n, cap_clusters < C -> MVICP_ERR_ARG; no mvicp_cluster before -> MVICP_ERR_STATE. */
int mvicp_cluster_fetch(mvicp_ctx* ctx, long long cap_n, int* label, unsigned char* core, long long cap_clusters, int* size);
/* Which clusters stay (pure host function, no context): the clusters are ranked by (size descending, label ascending), rank 0 first, and
 *   keep[c] = size[c] >= min_size && (max_clusters == 0 || rank(c) < max_clusters)     (1 / 0; n_clusters bytes)
 * Errors: a negative n_clusters, min_size or max_clusters, NULL size or keep -> MVICP_ERR_ARG. */
int mvicp_cluster_keep_rule(long long n_clusters, const int* size, long long min_size, long long max_clusters, unsigned char* keep);
/* Applies mvicp_cluster_keep_rule to the last mvicp_cluster result: the points with label >= 0 whose cluster is kept, in ascending original
 * index (noise always goes), compacted on the device.  The rows are the frame's stored bytes at the time of this call.  May be called again
 * with another rule; the selection lives as long as the mvicp_cluster result.  RETURNS THE NUMBER OF ROWS KEPT or a negative mvicp_status.
 * Errors: NULL context, min_size < 0, max_clusters < 0 -> MVICP_ERR_ARG; no mvicp_cluster result -> MVICP_ERR_STATE. */
long long mvicp_cluster_select(mvicp_ctx* ctx, long long min_size, long long max_clusters);
/* Copies the last selection: xyz / nrm (kept x 3 doubles: the stored bytes; nrm iff the frame has normals), idx (kept ints: original
 * indices, ascending), label (kept ints); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the context's device, decided
 * per pointer as mvicp_voxel_fetch decides, so a device result goes straight into mvicp_set_frame_device.  cap = rows each destination holds.
 * Errors: NULL context, cap < kept -> MVICP_ERR_ARG; no mvicp_cluster result, no mvicp_cluster_select of it, or nrm != NULL for a frame
 * without normals -> MVICP_ERR_STATE. */
int mvicp_cluster_fetch_kept(mvicp_ctx* ctx, long long cap, double* xyz, double* nrm, int* idx, int* label);

/* ---- plane segmentation: the dominant plane of one stored cloud by RANSAC, refitted over its inliers; plane out, then cluster --------
 * Objects stand on a table, a floor or a turntable, and that plane joins them into one cluster of mvicp_cluster; it is also the one thing
 * of a turntable scan that is the same in every view.  This stage names it.  The result is a pure function of the stored cloud
 * p_0 .. p_{n-1} of `frame` (the stored bytes in original order, finite by mvicp_set_frame's own check; no pose, no hash structure, no
 * graph) and of the arguments, bit for bit, whatever order the GPU's threads run in (tests/planeref.py is the same definition in numpy and
 * as a scalar loop): only comparisons, integer sums and a maximum cross lanes.  fp64, every operation rounded on its own, no fma;
 * dot(x, y) = (x0 y0 + x1 y1) + x2 y2 and cross(x, y) = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0), the forms of mvicp_consensus.
 *   Sample     hypothesis h (0 <= h < hypotheses), slot t in {0, 1, 2}: the generator of mvicp_consensus with c = n gives the index i_t.
 *              Two equal indices: the hypothesis is rejected.  The check precedes every load, so n < 3 rejects everything and is no error.
 *   Plane      a = p_{i0}, u = p_{i1} - a, v = p_{i2} - a, w = cross(u, v), nw = sqrt(dot(w, w)); rejected unless 0 < nw < +inf;
 *              m = w / nw, componentwise.
 *   Direction  only when `axis` is given (3 finite doubles, not all zero; cos_min in [0, 1]): da = dot(m, axis); rejected unless
 *              da * da >= (cos_min * cos_min) * dot(axis, axis).  The cosine, not an angle: no cos() enters the contract.
 *   Score      o_i = p_i - a, r_i = dot(m, o_i); point i is an inlier iff fabs(r_i) <= tau (inclusive).  count[h] = the number of
 *              inliers, -1 for a rejected hypothesis.  The offset from a is taken BEFORE the dot product, so the test keeps its meaning
 *              at UTM coordinates.
 *   Winner     the largest count, the lowest h among equals.  Nothing accepted: best = -1, count = 0, the plane all zeros, no flag set;
 *              that is no error.
 *   Refit      (refine != 0 and a winner exists) over the winner's inlier set I, c = |I|:
 *              omax = the maximum over I and the three axes of |o_i|; omax == 0: the refit is refused and the refined plane is the
 *                hypothesis, refit = 0.
 *              L = the bit length of c, b = min(21, (62 - L) / 2) in integer division, q = the integer with 2^(b-1) <= omax 2^q < 2^b.
 *              M_i = floor(ldexp(o_i, q)) componentwise, as int64; s_k = sum M_ik and S_kl = sum M_ik M_il (k <= l) are exact int64 sums
 *                (|s| < 2^(L+b), |S| < 2^(L+2b) <= 2^62).
 *              The rest is mvicp_plane_from_moments(c, s, S, q, a, m): C_kl = the 128-bit integer c S_kl - s_k s_l converted to double
 *                with round-to-nearest-even (as mvicp_outlier_threshold converts its 128-bit value); the Jacobi iteration of
 *                mvicp_estimate_normals on C with V = I (6 sweeps over (0,1), (0,2), (1,2); a rotation is skipped iff C[p][q] == 0); the
 *                index of the smallest diagonal entry by that contract's two strict comparisons; that column divided by its length;
 *                negated iff its dot product with m is < 0: the normal m'.  The point g_k = a_k + ldexp((double)s_k / (double)c + 0.5, -q)
 *                (the 0.5 undoes the floor's bias).
 *              Refined flags: fabs(dot(m', p_i - g)) <= tau; count_refined is their number.
 *   Output     the record below, count (hypotheses ints) and flags (n bytes): by the refined plane when refit == 1, otherwise by the
 *              hypothesis.  Without a refit normal / point repeat hyp_normal / hyp_point, count_refined = count and b = q = 0.
 *   Selection  mvicp_plane_select: the points with flag = 1 (the plane) or flag = 0 (the rest) in ascending original index, each with
 *              xyz, nrm (iff the frame has normals) and idx, as the stored bytes.
 * Repeated extraction is the caller's loop: select the rest, mvicp_set_frame_device, call again.  Left out: adaptive early termination
 * (count[h] is an output for every h), a point-normal agreement test per inlier, models other than a plane, sampling from a mask.
 * Needs 1 <= hypotheses <= 2^24 and a finite tau > 0.  HISTORY-NEUTRAL like mvicp_cluster: it does not modify the frame and leaves caches,
 * seeds, lists, epochs, medians, the AUTO state and queued evaluations alone.  With several ranks every rank computes it locally.  The call
 * returns when the result is complete; the result lives in library-owned device memory until the next mvicp_segment_plane, an upload to
 * `frame`, mvicp_set_num_frames or mvicp_destroy.  Profile scopes: "plane_hyp", "plane_score", "plane_pick", "plane_moments",
 * "plane_flags", "plane_compact".
 * Errors: NULL context or result, a frame index out of range, hypotheses outside [1, 2^24], a tau that is not finite or <= 0, an axis
 * that is not finite or all zero, cos_min outside [0, 1] (looked at only with an axis) -> MVICP_ERR_ARG, decided before the context is
 * touched: the previous result stays; a frame never uploaded -> MVICP_ERR_STATE. */
typedef struct mvicp_plane_result {
  int best, count, accepted;         /* the winning hypothesis (-1: none), its inliers, the hypotheses not rejected */
  int refit;                         /* 1: normal / point / flags are the refitted plane's */
  int count_refined;                 /* the flags set */
  int b, q;                          /* the refit's bit budget and scale exponent (0 without a refit) */
  int has_normals;                   /* the frame had stored normals at this call.  What mvicp_plane_fetch_kept gives is decided when
                                        mvicp_plane_select runs: nrm iff the frame has stored normals THEN (an adopt in between counts) */
  long long n;                       /* points of the frame */
  double normal[3], point[3], d;     /* the plane dot(normal, x) + d = 0 through point; d = -dot(normal, point) */
  double hyp_normal[3], hyp_point[3];/* the winning hypothesis's own m and a */
} mvicp_plane_result;
int mvicp_segment_plane(mvicp_ctx* ctx, int frame, long long hypotheses, unsigned long long seed, double tau, const double* axis /* may be NULL */,
                        double cos_min, int refine, mvicp_plane_result* result);
/* Copies the last result: count (hypotheses ints), flags (n bytes); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the
 * context's device, decided per pointer as mvicp_voxel_fetch decides.  cap_h / cap_n = entries count / flags hold (each looked at only
 * when its array is given).
 * Errors: NULL context, cap_h < hypotheses, cap_n < n -> MVICP_ERR_ARG; no mvicp_segment_plane before -> MVICP_ERR_STATE. */
int mvicp_plane_fetch(mvicp_ctx* ctx, long long cap_h, int* count, long long cap_n, unsigned char* flags);
/* The points of the last mvicp_segment_plane result with flag = 1 (inliers != 0: the plane) or flag = 0 (inliers == 0: the rest), in
 * ascending original index, compacted on the device (the compaction of mvicp_outlier_filter and mvicp_cluster_select).  The rows are the
 * frame's stored bytes.  May be called again with the other choice; the selection lives as long as the result.
 * RETURNS THE NUMBER OF ROWS or a negative mvicp_status.
 * Errors: NULL context -> MVICP_ERR_ARG; no mvicp_segment_plane result -> MVICP_ERR_STATE. */
long long mvicp_plane_select(mvicp_ctx* ctx, int inliers);
/* Copies the last selection: xyz / nrm (kept x 3 doubles: the stored bytes; nrm iff the frame has normals), idx (kept ints: original
 * indices, ascending); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the context's device, decided per pointer as
 * mvicp_voxel_fetch decides, so a device result goes straight into mvicp_set_frame_device.  cap = rows each destination holds.
 * Errors: NULL context, cap < kept -> MVICP_ERR_ARG; no mvicp_segment_plane result, no mvicp_plane_select of it, or nrm != NULL for a
 * frame without normals -> MVICP_ERR_STATE. */
int mvicp_plane_fetch_kept(mvicp_ctx* ctx, long long cap, double* xyz, double* nrm, int* idx);
/* The refit rule from the integer sums on (pure host function, no context): c = the number of inliers, s[3] = sum M_k, S[6] = sum M_k M_l
 * in the order 00 01 02 11 12 22, q = the scale exponent, a / m = the hypothesis's point and unit normal -> normal[3], point[3] as the
 * Refit paragraph above defines them.  The device part of a refit ends at the ten integers; this function finishes it.
 * Errors: c outside [1, 2^31), a NULL pointer, q outside [-1100, 1100], a non-finite a or m, a negative S_kk or
 * c S_kk - s_k s_k < 0 (not the sums of one set) -> MVICP_ERR_ARG. */
int mvicp_plane_from_moments(long long c, const long long s[3], const long long S[6], int q, const double a[3], const double m[3], double normal[3], double point[3]);

/* ---- boundary points: where one stored cloud ends, exactly specified; reject pairs on them ---------------------------------------------
 * For views that overlap only in part, source points outside the overlap find their nearest neighbour on the rim of the target and those
 * pairs pull the pose; Rusinkiewicz & Levoy ("Efficient Variants of the ICP Algorithm", section 3.4) reject pairs that contain boundary
 * points.  This stage names them: a point is on the boundary when, seen in its tangent plane, the directions to its neighbours leave an
 * angular gap of at least theta (the criterion of PCL's BoundaryEstimation and Open3D's compute_boundary_points).  The result is a pure
 * function of the stored bytes and the arguments, bit for bit, whatever order the GPU's threads run in (tests/boundref.py is the same
 * definition in numpy and as a scalar loop): only comparisons, a per-lane OR and a count cross lanes.  All arithmetic
 * is fp64, every operation rounded on its own, no fma; only + - x / sqrt, comparisons and negation occur.
 *   Normals N  source 0: the frame's stored normals; source 1: the nrm of the last mvicp_estimate_normals / mvicp_fit_normals, which must
 *              be for this frame and not dropped by an upload -- exactly as mvicp_orient_normals defines them.  A missing source ->
 *              MVICP_ERR_STATE.
 *   Row        row i of mvicp_knn_search(frame, NULL, max_nn, radius) in self mode, 3 <= max_nn <= 64; radius <= 0: the max_nn nearest,
 *              radius finite and > 0: the max_nn nearest within the radius.  c_i = cnt[i], position t holds neighbour j_t,
 *              d_t = p_{j_t} - p_i per component for t < c_i.  The point itself and exact duplicates are in the row.
 *   Unit normal  l = sqrt((N0 N0 + N1 N1) + N2 N2).  Point i is UNDECIDED (flag 0, open 0, valid 0) unless 0 < l < +inf and c_i >= 3 (a NaN
 *              fails the comparison).  Otherwise n = N / l, componentwise.
 *   Tangent frame  step 4 of the mvicp_fit_normals contract, word for word: from n alone, a = the index of the smallest |n_a|, the lowest
 *              index among equals; w = e_a x n written out: a = 0: w = (+0.0, -n2, n1); a = 1: w = (n2, +0.0, -n0); a = 2: w = (-n1, n0, +0.0).
 *              u = w / sqrt((w0 w0 + w1 w1) + w2 w2); v = n x u: v0 = n1 u2 - n2 u1, v1 = n2 u0 - n0 u2, v2 = n0 u1 - n1 u0.
 *   Directions  x_t = (d_t0 u0 + d_t1 u1) + d_t2 u2, y_t the same with v, r_t = sqrt(x_t x_t + y_t y_t).  Entry t is VALID iff t < c_i and
 *              0 < r_t < +inf (the point itself, its duplicates and neighbours straight along the normal are not).  Then
 *              ex_t = x_t / r_t, ey_t = y_t / r_t.
 *   Sector     a valid entry s lies in t's sector iff ex_t ey_s - ey_t ex_s > 0 and ex_t ex_s + ey_t ey_s > cos_gap: s is counter-clockwise
 *              of t by an angle in (0, theta), theta = acos(cos_gap).  The caller passes the cosine, so no acos or atan2 enters the
 *              contract; cos_gap is finite and lies in (-1, 1); both comparisons are strict, so a gap of exactly theta is a gap.
 *   Result     open[i] = the number of valid t whose sector holds no valid s; flag[i] = (open[i] > 0); valid[i] = the number of valid
 *              entries; used[i] = c_i.  flag is n bytes, open / valid / used n ints each, row i the ORIGINAL index i; n = 0 gives zero rows
 *              and is not an error.
 *   Selection  mvicp_boundary_select: the points with flag = 1 (the boundary) or flag = 0 (the rest, UNDECIDED points among them) in
 *              ascending original index, each with xyz, nrm (iff the frame has STORED normals, whatever the source was) and idx, as the
 *              stored bytes.
 * Negating N mirrors the plane (x -> -x exactly, y unchanged), which turns counter-clockwise into clockwise: a gap of at least theta
 * stays one, so flag is unchanged up to rounding exactly at the threshold; open may differ where a row has several gaps of which a
 * rounding decides one.  Nothing more is promised.  Left out: rows of every neighbour within a radius (a row is a wave), boundaries from
 * range-image structure, hole filling.
 * The call performs mvicp_knn_search(frame, NULL, max_nn, radius) internally and AFTERWARDS THAT SEARCH IS THE CONTEXT'S LAST
 * NEIGHBOUR-SEARCH RESULT, as with mvicp_estimate_normals.  Otherwise it is HISTORY-NEUTRAL: the result lives in a stage of its own, the
 * frame, its normals and the estimate it read are never touched; it needs the frame's hash structure (waits for pending builds and reports
 * a failed one the same way) and NO graph; with several ranks every rank computes it locally.  It returns when the result is complete; the
 * result lives in library-owned device memory until the next mvicp_boundary, an upload to the same frame, mvicp_set_num_frames or
 * mvicp_destroy.  Profile scopes: those of the search, "boundary"; of the selection "boundary_compact".
 * RETURNS THE NUMBER OF FLAGGED POINTS (>= 0) or a negative mvicp_status.
 * Errors: NULL context, a frame index out of range, a source outside {0, 1}, max_nn outside [3, 64], a non-finite radius, a cos_gap not
 * in (-1, 1) (a NaN is not) -> MVICP_ERR_ARG, decided before the context is touched (earlier results stay); a frame never uploaded, no
 * normals of the asked source -> MVICP_ERR_STATE (earlier results stay). */
long long mvicp_boundary(mvicp_ctx* ctx, int frame, int source, int max_nn, double radius, double cos_gap);
/* Copies the last result: flag (n bytes), open / valid / used (n ints each); each may be NULL; each may be a HOST pointer or a DEVICE
 * pointer of the context's device, decided per pointer as mvicp_voxel_fetch decides.  cap_rows = rows the destinations hold.
 * Errors: NULL context, cap_rows < n -> MVICP_ERR_ARG; no mvicp_boundary before -> MVICP_ERR_STATE. */
int mvicp_boundary_fetch(mvicp_ctx* ctx, long long cap_rows, unsigned char* flag, int* open, int* valid, int* used);
/* The points of the last mvicp_boundary result with flag = 1 (boundary != 0: the boundary points) or flag = 0 (boundary == 0: the rest), in
 * ascending original index, compacted on the device (the compaction of mvicp_outlier_filter, mvicp_cluster_select and mvicp_plane_select).
 * The rows are the frame's stored bytes.  May be called again with the other choice; the selection lives as long as the result.
 * RETURNS THE NUMBER OF ROWS or a negative mvicp_status.
 * Errors: NULL context -> MVICP_ERR_ARG; no mvicp_boundary result -> MVICP_ERR_STATE. */
long long mvicp_boundary_select(mvicp_ctx* ctx, int boundary);
/* Copies the last selection: xyz / nrm (kept x 3 doubles: the stored bytes; nrm iff the frame has normals), idx (kept ints: original
 * indices, ascending); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the context's device, decided per pointer as
 * mvicp_voxel_fetch decides, so a device result goes straight into mvicp_set_frame_device.  cap = rows each destination holds.
 * Errors: NULL context, cap < kept -> MVICP_ERR_ARG; no mvicp_boundary result, no mvicp_boundary_select of it, or nrm != NULL for a
 * frame without normals -> MVICP_ERR_STATE. */
int mvicp_boundary_fetch_kept(mvicp_ctx* ctx, long long cap, double* xyz, double* nrm, int* idx);

/* ---- reject masks: pairs that touch flagged points are dropped INSIDE the search ------------------------------------------------
 * A frame may carry a per-point reject mask (n bytes, ORIGINAL point order, nonzero = reject) that applies when the frame is the target
 * of an edge (MVICP_REJECT_AS_TARGET), its source (MVICP_REJECT_AS_SOURCE) or both.  A MASKED SEARCH is mvicp_correspond with this
 * acceptance test for query k of edge (s, d) whose nearest neighbour is j (original indices):
 *     accepted  <=>  j >= 0  &&  sqrt(d2) < thresh  &&  !(src_mask_s && src_mask_s[k])  &&  !(dst_mask_d && dst_mask_d[j])
 * The nearest neighbour itself is unchanged: a query whose neighbour is flagged is DROPPED, not re-matched to the next unflagged point
 * (Rusinkiewicz & Levoy 2001, section 3.4).  Counts, lists, stored distances, the upper median and the weight (float)(1.5 * median)
 * follow from the accepted set: they are what the unmasked search gives over the kept pairs alone (tests/rejectref.py is this
 * statement in numpy, and the search equals it byte for byte).  THE SCALE THEREFORE DIFFERS FROM THE HOST COMPOSITION (fetch the list,
 * filter it, mvicp_set_correspondences with the weight the search returned), which keeps the weight of the UNFILTERED list: here the
 * median is taken over what is kept -- the reference's rule applied to the list that exists.
 * The lists stay SEARCHED lists: the temporal NN cache, the in-place list upkeep, the fixed-point shortcuts and the queued evaluations
 * all keep working, and no list crosses the bus.  Everything downstream (the operand stream, the select, the export,
 * mvicp_normal_agreement, every objective) reads the filtered list.  Explicit lists (mvicp_set_correspondences) are never filtered.
 * With no mask on any frame every call behaves exactly as without this interface.
 * Setting, changing or clearing the mask of frame f voids the queued evaluations and makes every owned edge whose target (role TARGET)
 * or source (role SOURCE) is f re-compact and re-gather its list in the NEXT search, which gives it a new epoch; until that search the
 * lists on the device are the last search's.  The temporal NN cache stays valid: it is a fact about nearest neighbours, not about
 * lists.  Installing the same bytes again counts as a change.  mvicp_set_frame, mvicp_set_frame_device and mvicp_set_num_frames drop
 * the frame's mask with its cloud.
 * Sharded contexts: lists belong to their owner and counts are exchanged as before; THE CALLER OWES THE SAME MASKS ON EVERY RANK
 * BEFORE THE SAME SEARCH.  Unlike explicit lists, masks do not turn the queued evaluation ("spec_eval") off. */
enum { MVICP_REJECT_AS_TARGET = 1, MVICP_REJECT_AS_SOURCE = 2 };
/* mask: n bytes (n = the frame's points) in original point order, a HOST pointer or a DEVICE pointer of the context's device (decided
 * as mvicp_voxel_fetch decides); copied before the call returns.  mask NULL or roles == 0 clears the frame's mask.  Needs the frame's
 * structures (waits for pending builds) and NO graph.
 * Errors: NULL context, a frame out of range, roles outside [0, 3], a mask on another device -> MVICP_ERR_ARG; a frame never uploaded
 * or without structures -> MVICP_ERR_STATE.  All are decided before anything changes. */
int mvicp_set_reject_mask(mvicp_ctx* ctx, int frame, const unsigned char* mask, int roles);
/* The flags of the last mvicp_boundary become its frame's reject mask without leaving the device (the analogue of
 * mvicp_normals_adopt); roles == 0 clears that frame's mask.
 * Errors: NULL context, roles outside [0, 3] -> MVICP_ERR_ARG; no boundary result, or the frame was uploaded again since (the upload
 * dropped the result) -> MVICP_ERR_STATE, with nothing changed. */
int mvicp_boundary_adopt(mvicp_ctx* ctx, int roles);
/* Reads the frame's mask back: the caller's bytes in original order into out (HOST or DEVICE pointer; NULL: only the size), *roles
 * (may be NULL) = its roles.  RETURNS n, or 0 with *roles = 0 when the frame has no mask.
 * Errors: NULL context, a frame out of range, cap < n with out != NULL -> MVICP_ERR_ARG. */
long long mvicp_get_reject_mask(mvicp_ctx* ctx, int frame, unsigned char* out, long long cap, int* roles);

/* ---- neighbour search: the k nearest and / or all points within a radius, for arbitrary queries, with indices ------------
 * The search primitive of every point-cloud toolkit (search_knn, search_radius, the hybrid of the two) over one stored cloud.  The result
 * is a pure function of the inputs, bit for bit (tests/knnref.py is the same definition in numpy):
 *   Inputs     the stored cloud p_0 .. p_{n-1} of `frame` (the stored bytes, no pose); queries: m x 3 doubles in the frame's local
 *              coordinates, like mvicp_nn_query.  `queries` may be a HOST pointer or a DEVICE pointer of the context's device, decided per
 *              pointer as mvicp_voxel_fetch decides (another device's memory is MVICP_ERR_ARG); a device array must be fully written when
 *              the call is made.  queries == NULL is SELF MODE: m is ignored, row i is the neighbourhood of p_i, i an ORIGINAL index, and
 *              the point itself is an ordinary candidate with d2 = +0.
 *   Metric     dist2 of csrc/nn_metric.h: (d0 d0 + d1 d1) + d2 d2 with d = q - p, every operation rounded on its own, no fma.
 *   Radius     on iff radius > 0: j is a candidate of query i iff sqrt(dist2(q_i, p_j)) < radius (IEEE sqrt, strict) -- the predicate of
 *              mvicp_outlier_filter; equivalently dist2 < B2, B2 as defined at mvicp_overlap.  Radius off: every j is a candidate.
 *   Order      the candidates of a query are ordered by (dist2 ascending, ORIGINAL index j ascending).  This is deliberately NOT the
 *              nanoflann visiting order of mvicp_recompute_normals' knn_out: that order exists to reproduce the reference and needs the
 *              reference's own tree over the cloud; this one is a pure function of the cloud, no tie tree is built or needed, and among
 *              equidistant points the lowest original indices win.
 *   k mode     1 <= k <= 64: cnt[i] = min(k, number of candidates); row i of idx / d2 (dense m x k) holds the first cnt[i] candidates, the
 *              rest of the row is padded with idx = -1, d2 = +inf; off, if asked for, gets the m + 1 entries i k.
 *   All mode   k == 0 (needs radius > 0): every candidate, in CSR form: off[0] = 0, off[i+1] = off[i] + cnt[i]; idx / d2 have off[m]
 *              entries.  A row is put in order by one GPU wave in O(len^2 / 64): rows of thousands of entries (a radius as large as the
 *              cloud) are correct, not fast.
 *   Empty      an empty frame (n = 0) gives every cnt[i] = 0 and is not an error; m = 0 gives an empty result.
 *   Anywhere   queries may lie anywhere, far outside the cloud included; those in empty space are exact, not fast.
 * Needs the frame's hash structure (waits for pending builds and reports a failed one, like mvicp_overlap), NO graph, and is
 * HISTORY-NEUTRAL: it leaves caches, seeds, lists, epochs, medians, the AUTO state, queued evaluations and tie_skip alone and builds no tie
 * tree, so a registration with searches in between is bit-identical to one without.  With several ranks every rank computes it locally.
 * The call returns when the result is complete; the result lives in library-owned device memory until the next mvicp_knn_search,
 * mvicp_set_num_frames or mvicp_destroy.  Option "knn_order" (default 1; 0 = answer the queries in the order given instead of the order of
 * their hash cells) changes the speed only: the result is the same bytes.  Profile scopes: "knn_key", "knn_search", "knn_count",
 * "knn_fill", "knn_order".
 * RETURNS THE NUMBER OF ENTRIES sum cnt[i] (>= 0) or a negative mvicp_status.
 * Errors: NULL context, k outside [0, 64], a non-finite radius, k == 0 with radius <= 0, m < 0 or m >= 2^31 with queries given, a frame
 * index out of range -> MVICP_ERR_ARG, decided before the context is touched; a frame never uploaded -> MVICP_ERR_STATE; a non-finite query
 * coordinate, a stored neighbour distance that overflowed to +inf, an all-mode total >= 2^31 -> MVICP_ERR_ARG, reported by this call, and
 * no result is left behind.  An argument error of the first kind leaves the previous result alone. */
long long mvicp_knn_search(mvicp_ctx* ctx, int frame, const double* queries, long long m, int k, double radius);
/* Copies the last result: cnt (m ints), off (m + 1 long long), idx (ints) / d2 (doubles) with m k entries (k mode) or off[m] (all mode);
 * each may be NULL; each may be a HOST pointer or a DEVICE pointer of the context's device, decided per pointer as mvicp_voxel_fetch
 * decides.  cap_rows = rows cnt holds (off holds one more), looked at only when cnt or off is given; cap_entries = entries idx / d2 hold,
 * looked at only when one of the two is given.
 * Errors: NULL context, cap_rows < m, cap_entries too small -> MVICP_ERR_ARG; no mvicp_knn_search before -> MVICP_ERR_STATE. */
int mvicp_knn_fetch(mvicp_ctx* ctx, long long cap_rows, long long cap_entries, int* cnt, long long* off, int* idx, double* d2);

/* ---- FPFH surface descriptors (Rusu 2009), exactly specified ----------------------------------------------------------------
 * The 33-bin Fast Point Feature Histogram of every point of one stored cloud with normals: the link between "downsample + normals" and
 * "match + coarse pose" of every registration pipeline.  The result is a pure function of the stored bytes, bit for bit
 * (tests/fpfhref.py is the same definition in numpy and as a scalar loop).  The textbook formulas use atan2 and acos, which no library
 * rounds correctly; the contract states the same geometry with + - x / sqrt, comparisons and floor only, in fp64, every operation rounded
 * on its own, no fma:
 *   Inputs     the stored cloud p_0 .. p_{n-1} and normals n_0 .. n_{n-1} of `frame` (the stored bytes, no pose; the normals are used as
 *              given, they are not normalised), radius > 0, 2 <= max_nn <= 64.
 *   N(i)       row i of mvicp_knn_search(frame, NULL, max_nn, radius) -- self mode, the max_nn nearest within the radius, in the order
 *              (dist2, original index) -- without its entries with d2 == 0 (the point itself and exact duplicates, whose pair frame is
 *              undefined); m_i = |N(i)| <= 63.
 *   Pair       j in N(i): d = p_j - p_i, dist = sqrt(d2) with the row's d2; dot products (x0 y0 + x1 y1) + x2 y2, cross products
 *              componentwise x1 y2 - x2 y1, ...; a1 = n_i . d, a2 = n_j . d.  |a1| < |a2| (ties do not swap): s = n_j, t = n_i, e = -d,
 *              f3 = (-a2) / dist; otherwise s = n_i, t = n_j, e = d, f3 = a1 / dist.  v = e x s, vn = sqrt(v . v); vn == 0: the pair's
 *              three bins are (5, 5, 5); otherwise v = v / vn, w = s x v, f2 = v . t, y = w . t, x = s . t.
 *   Bins       11 each.  f2, f3: min(10, max(0, floor((f + 1.0) * 5.5))).  theta = the angle of (x, y) in (-pi, pi]: its bin is the number
 *              of inner edges phi_k = -pi + 2 pi k / 11, k = 1 .. 10, it has passed, decided with the doubles (c_k, s_k) nearest to
 *              (cos phi_k, sin phi_k) and cr_k = c_k * y - s_k * x: an edge k <= 5 is passed iff y >= 0 or cr_k >= 0, an edge k >= 6 iff
 *              (y > 0 and cr_k >= 0) or (y == 0 and x < 0).
 *   SPFH       integer counts c_i[33] over N(i): theta bins 0-10, f2 bins 11-21, f3 bins 22-32; r_i = 100.0 / (double)m_i, 0 if m_i == 0.
 *   FPFH       acc[b] = +0.0; over N(i) IN ROW ORDER: g = r_j / d2, acc[b] = acc[b] + (double)c_j[b] * g.  Per sub-histogram S = the
 *              sequential sum of its 11 acc in ascending b, scale = 100.0 / S if S != 0 else 0;
 *              desc[i][b] = acc[b] * scale + (double)c_i[b] * r_i.  A point with m_i == 0 gets the all-zero row.
 * desc is n x 33 doubles and used holds m_i, row i the ORIGINAL index i; n = 0 gives zero rows and is not an error.
 * The call performs mvicp_knn_search(frame, NULL, max_nn, radius) internally and AFTERWARDS THAT SEARCH IS THE CONTEXT'S LAST
 * NEIGHBOUR-SEARCH RESULT: mvicp_knn_fetch returns the neighbourhoods the descriptors were computed over, at no extra cost, and the
 * previous search result is gone.  Otherwise the call is HISTORY-NEUTRAL like mvicp_knn_search, needs the frame's hash structure (waits
 * for pending builds and reports a failed one the same way) and NO graph; with several ranks every rank computes it locally.  It returns
 * when the result is complete; the result lives in library-owned device memory until the next mvicp_fpfh, mvicp_set_num_frames or
 * mvicp_destroy.  Profile scopes: those of the search, "fpfh_spfh", "fpfh_sum".
 * RETURNS THE NUMBER OF ROWS n (>= 0) or a negative mvicp_status.
 * Errors: NULL context, max_nn outside [2, 64], a radius that is not finite or <= 0, a frame index out of range -> MVICP_ERR_ARG, decided
 * before the context is touched (earlier results stay); a frame never uploaded, or uploaded without normals -> MVICP_ERR_STATE. */
long long mvicp_fpfh(mvicp_ctx* ctx, int frame, double radius, int max_nn);
/* Copies the last result: desc (n x 33 doubles), used (n ints: m_i); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the
 * context's device, decided per pointer as mvicp_voxel_fetch decides.  cap_rows = rows the destinations hold.
 * Errors: NULL context, cap_rows < n -> MVICP_ERR_ARG; no mvicp_fpfh before -> MVICP_ERR_STATE. */
int mvicp_fpfh_fetch(mvicp_ctx* ctx, long long cap_rows, double* desc, int* used);

/* ---- ISS keypoints (Zhong 2009), exactly specified ---------------------------------------------------------------------------------
 * Intrinsic Shape Signatures of one stored cloud: the few per cent of its points whose neighbourhood varies in all three directions and
 * whose smallest variance is a local maximum -- the stage between "normals" and "describe" that lets the descriptor match shrink by the
 * square of that fraction while the descriptors keep their full-resolution neighbourhoods.  The result is a pure function of the stored
 * bytes, bit for bit (tests/issref.py is the same definition in numpy and as a scalar loop).  All arithmetic is fp64, every operation
 * rounded on its own, no fma; only + - x / sqrt, floor, comparisons and integer arithmetic occur:
 *   Inputs     the stored cloud p_0 .. p_{n-1} of `frame` (the stored bytes, no pose; normals are not needed); both radii finite and in
 *              [2^-300, 2^300]; gamma21 and gamma32 finite and > 0 (usually 0.975); 1 <= min_neighbors <= 1024.
 *   N_r(i)     { j : sqrt(dist2(p_i, p_j)) < r }: the candidate set of a self-mode mvicp_knn_search row -- the same metric, the strict
 *              predicate on the correctly rounded sqrt, the point itself and exact duplicates included.  c_i = |N_salient(i)|,
 *              n_i = |N_nonmax(i)|.  Any c_i > 1024 -> MVICP_ERR_ARG, reported by this call; no result is left behind.
 *   Moments    exact integers, so the order in which the neighbours are added is free.  salient_radius = f 2^e with f in [0.5, 1)
 *              (frexp), q = 20 - e.  Per neighbour and component g = (int64) floor((p_j - p_i) * 2^q): the subtraction rounded, the
 *              scaling a multiplication by the double 2^q; |g| <= 2^20 + 1.  m_a = sum g_a, S_ab = sum g_a g_b,
 *              D_ab = c_i S_ab - m_a m_b; every integer stays below 2^62 in magnitude (c_i <= 2^10 gives c_i S_ab < 2^61 and
 *              |m_a m_b| < 2^62; D is c_i^2 times a covariance, so |D_ab| <= max_a c_i S_aa).
 *              C_ab = (double)D_ab / (double)(c_i c_i): one round-to-nearest-even conversion, an exact divisor, one division.
 *   Eigenvalues  A = the full 3 x 3 matrix of C.  Exactly 6 sweeps, no early exit, each over (p, q) = (0,1), (0,2), (1,2) in that order.
 *              A rotation is skipped iff A[p][q] == 0; otherwise theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]),
 *              t = (theta >= 0 ? 1.0 : -1.0) / (|theta| + sqrt(theta * theta + 1.0)), c = 1.0 / sqrt(t * t + 1.0), s = t * c; for r = 0, 1,
 *              2: (A[r][p], A[r][q]) <- (c * A[r][p] - s * A[r][q], s * A[r][p] + c * A[r][q]); then for r = 0, 1, 2:
 *              (A[p][r], A[q][r]) <- (c * A[p][r] - s * A[q][r], s * A[p][r] + c * A[q][r]).  l1 >= l2 >= l3 = the diagonal, sorted.
 *   Saliency   i is salient iff c_i >= min_neighbors, l2 < gamma21 * l1, l3 < gamma32 * l2 and l3 > 0; saliency[i] = l3 * 2^(-2q) (a
 *              multiplication by that double), +0.0 otherwise.
 *   Keypoints  i is a keypoint iff saliency[i] > 0, n_i >= min_neighbors and no j in N_nonmax(i) beats it; j beats i iff
 *              saliency[j] > saliency[i], or saliency[j] == saliency[i] and j < i (the lowest index wins a tie: exact duplicates give
 *              one keypoint).
 * idx holds the keypoints as ORIGINAL indices, ascending; saliency, cnt_salient (c_i) and cnt_nms (n_i) have n entries, by original index.
 * n = 0 gives no keypoint and is not an error.  The call is HISTORY-NEUTRAL like mvicp_knn_search, needs the frame's hash structure (waits
 * for pending builds and reports a failed one the same way) and NO graph; with several ranks every rank computes it locally.  It returns
 * when the result is complete; the result lives in library-owned device memory of its own (the last results of mvicp_knn_search,
 * mvicp_fpfh, mvicp_feature_match, mvicp_consensus and mvicp_coarse_pairs are left untouched) until the next mvicp_iss_keypoints,
 * mvicp_set_num_frames or mvicp_destroy.  Profile scopes: "iss_moments", "iss_nms", "iss_compact".
 * RETURNS THE NUMBER OF KEYPOINTS (>= 0) or a negative mvicp_status.
 * Errors: NULL context, a radius outside [2^-300, 2^300] or not finite, a gamma that is not finite or <= 0, min_neighbors outside
 * [1, 1024], a frame index out of range -> MVICP_ERR_ARG, decided before the context is touched (earlier results stay); a frame never
 * uploaded -> MVICP_ERR_STATE. */
long long mvicp_iss_keypoints(mvicp_ctx* ctx, int frame, double salient_radius, double non_max_radius, double gamma21, double gamma32,
                              int min_neighbors);
/* Copies the last result: idx (k ints), xyz and nrm (k x 3 doubles: the stored rows at idx), saliency (n doubles), cnt_salient and cnt_nms
 * (n ints); each may be NULL; each may be a HOST pointer or a DEVICE pointer of the context's device, decided per pointer as
 * mvicp_voxel_fetch decides.  cap_keys = keypoints the first three hold, cap_n = points the last three hold; each is looked at only
 * when one of its destinations is given.
 * Errors: NULL context, a cap too small -> MVICP_ERR_ARG; no mvicp_iss_keypoints before, nrm asked of a frame without normals ->
 * MVICP_ERR_STATE. */
int mvicp_iss_fetch(mvicp_ctx* ctx, long long cap_keys, int* idx, double* xyz, double* nrm, long long cap_n, double* saliency, int* cnt_salient,
                    int* cnt_nms);

/* ---- Normals with curvature, oriented to a viewpoint, exactly specified --------------------------------------------------------------
 * The stage between "clean cloud" and "describe / register on planes": per point the direction of least variance of its neighbourhood,
 * turned towards a viewpoint, and the surface variation.  Unlike mvicp_recompute_normals (the reference's recomputeNormals: k <= 16,
 * nanoflann's tie order, n_z <= 0, agreement to rounding) the result is a pure function of the stored bytes, bit for bit
 * (tests/normref.py is the same definition in numpy and as a scalar loop), and orienting the normals of several clouds consistently --
 * which FPFH and the symmetric objective depend on -- is the viewpoint's job: pass the sensor position of each view in that view's own
 * coordinates.  All arithmetic is fp64, every operation rounded on its own, no fma; only + - x / sqrt, comparisons and negation occur
 * (DESIGN.md section 3.14):
 *   Inputs     the stored cloud p_0 .. p_{n-1} of `frame` (the stored bytes, no pose); 3 <= max_nn <= 64; radius <= 0: the max_nn nearest,
 *              radius finite and > 0: the max_nn nearest within the radius; viewpoint: 3 finite doubles in the frame's local coordinates,
 *              NULL = (0, 0, 0), the sensor origin of a view in its own frame.
 *   N(i)       row i of mvicp_knn_search(frame, NULL, max_nn, radius) -- self mode, the order (dist2, original index), the point itself
 *              and exact duplicates included; c_i = cnt[i], position t of the row holds neighbour j_t.
 *   Offsets    d_t = p_{j_t} - p_i per component for t < c_i, +0.0 for c_i <= t < 64.  (Offsets from the point itself: a coordinate that
 *              all neighbours share then cancels exactly.)
 *   Tree sum   T(y) of 64 values: six times y[u] <- y[2u] + y[2u+1] (u = 0 .. half the length - 1); T(y) = y[0].  The order is part of
 *              the contract.
 *   Moments    mean_a = T(d_a) / (double)c_i; x_{t,a} = d_{t,a} - mean_a for t < c_i, else +0.0; C_ab = T(x_a * x_b) for a <= b, mirrored.
 *   Eigenvectors  A = C, V = the identity.  The Jacobi iteration of mvicp_iss_keypoints: exactly 6 sweeps, no early exit, each over
 *              (p, q) = (0,1), (0,2), (1,2) in that order.  A rotation is skipped iff A[p][q] == 0; otherwise
 *              theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]), t = (theta >= 0 ? 1.0 : -1.0) / (|theta| + sqrt(theta * theta + 1.0)),
 *              c = 1.0 / sqrt(t * t + 1.0), s = t * c; for r = 0, 1, 2: (A[r][p], A[r][q]) <- (c * A[r][p] - s * A[r][q],
 *              s * A[r][p] + c * A[r][q]); then for r = 0, 1, 2: (A[p][r], A[q][r]) <- (c * A[p][r] - s * A[q][r], s * A[p][r] + c * A[q][r]);
 *              then for r = 0, 1, 2: (V[r][p], V[r][q]) <- (c * V[r][p] - s * V[r][q], s * V[r][p] + c * V[r][q]).
 *   Normal     m = 0; if A[1][1] < A[m][m] then m = 1; if A[2][2] < A[m][m] then m = 2.  v = V[:, m], len = sqrt((v0 v0 + v1 v1) + v2 v2),
 *              n = v / len.
 *   Orientation  w = viewpoint - p_i, s = (n0 w0 + n1 w1) + n2 w2.  s < 0: every component of n is negated (a +0.0 becomes -0.0);
 *              s == 0 keeps n.
 *   Curvature  the surface variation: S = (A[0][0] + A[1][1]) + A[2][2], l = A[m][m]; curvature = l / S if l > 0 and S > 0, else +0.0.
 *   Too few    c_i < 3: normal (+0.0, +0.0, +0.0), curvature +0.0.  used[i] = c_i in every case.
 * nrm is n x 3 doubles, curvature n doubles, used n ints, row i the ORIGINAL index i; n = 0 gives zero rows and is not an error.  Rows of
 * every neighbour within a radius (k = 0, unbounded length) are not offered: the tree has 64 leaves.
 * The call performs mvicp_knn_search(frame, NULL, max_nn, radius) internally and AFTERWARDS THAT SEARCH IS THE CONTEXT'S LAST
 * NEIGHBOUR-SEARCH RESULT, as with mvicp_fpfh.  Otherwise the call is HISTORY-NEUTRAL like mvicp_knn_search -- it does NOT touch the
 * frame's normals -- needs the frame's hash structure (waits for pending builds and reports a failed one the same way) and NO graph; with
 * several ranks every rank computes it locally.  It returns when the result is complete; the result lives in library-owned device memory
 * of its own until the next mvicp_estimate_normals, an upload (mvicp_set_frame / mvicp_set_frame_device) to the same frame,
 * mvicp_set_num_frames or mvicp_destroy.  Profile scopes: those of the search, "normals_pca".
 * RETURNS THE NUMBER OF ROWS n (>= 0) or a negative mvicp_status.
 * Errors: NULL context, max_nn outside [3, 64], a non-finite radius, a non-finite viewpoint entry, a frame index out of range ->
 * MVICP_ERR_ARG, decided before the context is touched (earlier results stay); a frame never uploaded -> MVICP_ERR_STATE. */
long long mvicp_estimate_normals(mvicp_ctx* ctx, int frame, int max_nn, double radius, const double* viewpoint);
/* Copies the last result: nrm (n x 3 doubles), curvature (n doubles), used (n ints: c_i); each may be NULL; each may be a HOST pointer or a
 * DEVICE pointer of the context's device, decided per pointer as mvicp_voxel_fetch decides.  cap_rows = rows the destinations hold.
 * Errors: NULL context, cap_rows < n -> MVICP_ERR_ARG; no mvicp_estimate_normals before -> MVICP_ERR_STATE. */
int mvicp_normals_fetch(mvicp_ctx* ctx, long long cap_rows, double* nrm, double* curvature, int* used);
/* The frame of the last mvicp_estimate_normals takes that result's nrm as its normals.  In every observable this is what a successful
 * mvicp_recompute_normals leaves for those values: the frame's original-order and sorted normals are written (allocated if the frame was
 * uploaded without normals: point-to-plane and symmetric evaluation then accept it), every owned correspondence list that points into the
 * frame is re-gathered, queued evaluations are voided.  The result stays fetchable afterwards.  With several ranks every rank calls it
 * (after its own mvicp_estimate_normals); there is no communication.
 * Errors: NULL context -> MVICP_ERR_ARG; no result, or the frame was uploaded again since the estimate (the upload dropped the result) ->
 * MVICP_ERR_STATE, with nothing changed. */
int mvicp_normals_adopt(mvicp_ctx* ctx);

/* ---- Jet-fitted normals (osculating polynomial), exactly specified -----------------------------------------------------------------------
 * A PCA normal is the normal of the best plane through a curved, unevenly sampled patch.  mvicp_fit_normals fits a height polynomial of
 * degree 2 or 3 over the PCA tangent plane (an osculating jet, Cazals & Pouget 2005) and takes the gradient of that polynomial at the
 * point.  The result is a pure function of the stored bytes, bit for bit (tests/jetref.py is the same definition in numpy and as a scalar
 * loop).  All arithmetic is fp64, every operation rounded on its own, no fma; only + - x / sqrt, comparisons and
 * negation occur.  Arguments other than `degree` are those of mvicp_estimate_normals; the coordinates are finite and no product below
 * overflows.
 *   1 PCA      n (unit, oriented to the viewpoint), curvature and used = c_i exactly as mvicp_estimate_normals defines them, with that
 *              contract's row, offsets d_t = p_{j_t} - p_i (+0.0 for t >= c_i) and tree sum T.
 *   2 Basis    the monomials b_0 .. b_{M-1} = 1, X, Y, X2, XY, Y2 (degree 2, M = 6), continued by X3, X2Y, XY2, Y3 (degree 3, M = 10).
 *   3 Fallback the point keeps step 1's bytes unchanged, fitted = 0, if c_i < M, if h == 0 (step 5), if a pivot fails (step 8), or if a
 *              component of g or its length is not finite or the length is 0 (step 10).  Otherwise fitted = 1.
 *   4 Frame    from n alone: a = the index of the smallest |n_a|, the lowest index among equals; w = e_a x n written out:
 *              a = 0: w = (+0.0, -n2, n1); a = 1: w = (n2, +0.0, -n0); a = 2: w = (-n1, n0, +0.0).
 *              u = w / sqrt((w0 w0 + w1 w1) + w2 w2); v = n x u: v0 = n1 u2 - n2 u1, v1 = n2 u0 - n0 u2, v2 = n0 u1 - n1 u0.
 *   5 Scale    h2 = the largest (d_t0 d_t0 + d_t1 d_t1) + d_t2 d_t2 over t < c_i; h = sqrt(h2).
 *   6 Coordinates  for t < c_i: X_t = ((d_t0 u0 + d_t1 u1) + d_t2 u2) / h, Y_t the same with v, Z_t the same with n; X2 = X * X, XY = X * Y,
 *              Y2 = Y * Y, X3 = X2 * X, X2Y = X2 * Y, XY2 = X * Y2, Y3 = Y2 * Y; b_0 = 1.0.  For t >= c_i every b_m and Z are +0.0.
 *   7 Normal equations  G_ml = T(b_m * b_l) for m <= l (mirrored), r_m = T(b_m * Z).
 *   8 Cholesky  for j = 0 .. M-1: s = G_jj, then for q = 0 .. j-1 ascending s <- s - L_jq * L_jq; the pivot fails unless
 *              s > 2^-20 * G_jj (a NaN fails); L_jj = sqrt(s); for r = j+1 .. M-1: s = G_rj, then for q = 0 .. j-1 ascending
 *              s <- s - L_rq * L_jq; L_rj = s / L_jj.  The threshold 2^-20 is part of the contract.
 *   9 Solves   forward, j = 0 .. M-1: s = r_j, for q = 0 .. j-1 ascending s <- s - L_jq * y_q; y_j = s / L_jj.  Back, m = M-1 .. 1:
 *              s = y_m, for q = M-1 .. m+1 descending s <- s - L_qm * a_q; a_m = s / L_mm.  a_0 (the height at the point) is NOT computed.
 *  10 Normal   g_b = (n_b - a_1 * u_b) - a_2 * v_b; len = sqrt((g0 g0 + g1 g1) + g2 g2); nrm = g / len.  No re-orientation: g . n is 1 up
 *              to rounding.
 * The curvature stays the PCA surface variation of step 1.  THE RESULT REPLACES THE CONTEXT'S LAST mvicp_estimate_normals RESULT: the same
 * slot, so mvicp_normals_fetch, mvicp_normals_adopt and mvicp_orient_normals(source = 1) act on it unchanged, and its lifetime and drop
 * rules are the estimate's (the next mvicp_estimate_normals or mvicp_fit_normals, an upload to the frame, mvicp_set_num_frames,
 * mvicp_destroy).  In addition it holds one byte per point, fitted, for mvicp_normals_fit_fetch.  Like the estimate the call leaves its
 * internal search as the context's last neighbour search, is otherwise HISTORY-NEUTRAL and needs NO graph.  Profile scopes: those of the
 * search, "normals_jet".
 * RETURNS THE NUMBER OF ROWS n (>= 0) or a negative mvicp_status.
 * Errors: those of mvicp_estimate_normals, and a degree outside {2, 3} -> MVICP_ERR_ARG; argument errors are decided before the context
 * is touched (earlier results stay). */
long long mvicp_fit_normals(mvicp_ctx* ctx, int frame, int max_nn, double radius, const double* viewpoint, int degree);
/* Copies the fitted bytes (n unsigned chars, 1 = the row is the fit, 0 = the row is the PCA estimate) of the last mvicp_fit_normals; a
 * HOST pointer or a DEVICE pointer of the context's device, decided as mvicp_voxel_fetch decides; may be NULL.  cap_rows = rows the
 * destination holds.
 * Errors: NULL context, cap_rows < n -> MVICP_ERR_ARG; the context's last estimate is not a mvicp_fit_normals result, or there is none ->
 * MVICP_ERR_STATE. */
int mvicp_normals_fit_fetch(mvicp_ctx* ctx, long long cap_rows, unsigned char* fitted);

/* ---- Jet smoothing and surface curvatures, exactly specified -----------------------------------------------------------------------------
 * No other stage moves a point, so sensor noise along the surface normal reaches the normals, the descriptors, the objective and the fused
 * model unchanged.  mvicp_smooth_points continues the fit of mvicp_fit_normals by one row of its back substitution, to a_0: the height of
 * the fitted polynomial at the point, i.e. the distance from the point to the fitted surface along the PCA normal.  It moves the point there
 * (CGAL's jet_smooth_point_set, the unweighted form of moving least squares) and reports the mean and the Gaussian curvature of the
 * polynomial at the point, which do not depend on the choice of (u, v).  The result is a pure function of the stored bytes, bit for bit
 * (tests/smoothref.py is the same definition in numpy and as a scalar loop).  Steps 1 to 10 of mvicp_fit_normals
 * apply word for word, with the same arithmetic rules: fp64, every operation rounded on its own, no fma; only + - x / sqrt, comparisons and
 * negation occur.  "Fitted" below means fitted = 1 after step 10.  Added are:
 *   9a Height  the back substitution goes on to m = 0: s = y_0, for q = M-1 .. 1 descending s <- s - L_q0 * a_q; a_0 = s / L_00.
 *  11 Shift    shift = a_0 * h where the row is fitted and that product is finite, else +0.0.
 *  12 Projection  x'_b = p_b + shift * n_b for b = 0, 1, 2, with n the PCA normal of step 1 (not the fitted normal), one product and one sum
 *              per component.  moved = 1 iff the row is fitted, a_0 * h is finite, (max_shift <= 0 or |shift| <= max_shift) and all three
 *              x'_b are finite; then xyz = x'.  Otherwise moved = 0 and xyz holds p_i's bytes.  shift is reported either way.
 *  13 Curvatures  where the row is fitted: E = 1.0 + a_1 * a_1, G = 1.0 + a_2 * a_2, F = a_1 * a_2, w2 = E + a_2 * a_2, w = sqrt(w2),
 *              zxx = (a_3 + a_3) / h, zxy = a_4 / h, zyy = (a_5 + a_5) / h,
 *              H = ((G * zxx - (F + F) * zxy) + E * zyy) / ((w2 * w) + (w2 * w)), K = (zxx * zyy - zxy * zxy) / (w2 * w2).
 *              H is positive where the surface bends towards n: a sphere seen from outside has H = -1/R, K = 1/R^2.  If the row is not
 *              fitted, or H or K is not finite, both are +0.0.  No NaN reaches an output.
 * Arguments: those of mvicp_fit_normals, and max_shift: <= 0 means no limit, +inf is allowed.
 * nrm, curvature, used and fitted are exactly mvicp_fit_normals' bytes and live in that call's slot: mvicp_normals_fetch,
 * mvicp_normals_fit_fetch, mvicp_normals_adopt and mvicp_orient_normals(source = 1) act on them unchanged.  xyz (n x 3 doubles), shift
 * (n doubles), moved (n bytes), H and K (n doubles each) live in a slot of their own with the same lifetime and drop rules; a later
 * mvicp_estimate_normals or mvicp_fit_normals drops them.  The frame's stored cloud is NOT changed: smoothing repeatedly is the caller's
 * loop (fetch xyz, and nrm if wanted, into device memory, mvicp_set_frame_device, call again).  Like the fit the call leaves its internal
 * search as the context's last neighbour search, is otherwise HISTORY-NEUTRAL and needs NO graph; with several ranks every rank computes
 * it locally.  Profile scopes: those of the search, "jet_smooth".
 * RETURNS THE NUMBER OF ROWS n (>= 0) or a negative mvicp_status.
 * Errors: those of mvicp_fit_normals, and a NaN max_shift -> MVICP_ERR_ARG; argument errors are decided before the context is touched
 * (earlier results stay). */
long long mvicp_smooth_points(mvicp_ctx* ctx, int frame, int max_nn, double radius, const double* viewpoint, int degree, double max_shift);
/* Copies the last mvicp_smooth_points result: xyz (n x 3 doubles), shift (n doubles), moved (n bytes), H, K (n doubles each); each may be
 * NULL; each may be a HOST pointer or a DEVICE pointer of the context's device, decided per pointer as mvicp_voxel_fetch decides, so xyz
 * goes straight into mvicp_set_frame_device.  cap_rows = rows the destinations hold.
 * Errors: NULL context, cap_rows < n -> MVICP_ERR_ARG; the context's last estimate is not a mvicp_smooth_points result, or there is none ->
 * MVICP_ERR_STATE. */
int mvicp_smooth_fetch(mvicp_ctx* ctx, long long cap_rows, double* xyz, double* shift, unsigned char* moved, double* H, double* K);

/* ---- Consistent normal orientation without a viewpoint: propagation over a neighbour graph ----------------------------------------
 * mvicp_estimate_normals turns a normal towards a viewpoint, which is right for a range image and for nothing else.  mvicp_orient_normals
 * makes the normals of ONE cloud agree with each other without one (Hoppe et al. 1992): the sign is carried along the maximum spanning
 * forest of the neighbour graph weighted by |N_i . N_j|.  The result is a pure function of the stored bytes, bit for bit
 * (tests/orientref.py is the same definition in numpy and as a scalar Kruskal loop).  All floating-point work is
 * fp64, every operation rounded on its own, no fma; comparisons are IEEE as written.
 *   Normals N   source 0: the frame's stored normals (none: MVICP_ERR_STATE); source 1: the nrm of the last mvicp_estimate_normals, which
 *              must be for this frame and not dropped by an upload (otherwise MVICP_ERR_STATE).
 *   Graph      the rows of mvicp_knn_search(frame, NULL, k, radius) in self mode, 2 <= k <= 64, radius <= 0: off.  The undirected edge
 *              {i, j}, i != j, exists iff j is in row i or i is in row j.  Exact duplicates are ordinary points.
 *   Weight     d_ij = (N_i0 N_j0 + N_i1 N_j1) + N_i2 N_j2 (bitwise symmetric in i and j), w = |d|, f_ij = [d < 0].  A non-finite d ->
 *              MVICP_ERR_ARG, reported by this call, and no result is left behind.  Zero normals (rows of fewer than 3 points) give
 *              w = 0, f = 0 and take part like any other.
 *   Forest     edge e precedes e' iff w_e > w_e', for equal w iff its (min index, max index) is lexicographically smaller: a strict total
 *              order, so the maximum spanning forest F -- the one Kruskal builds in that order -- is unique, whatever algorithm builds it.
 *   Labels     comp[i] = the lowest original index in i's tree (its anchor); x_i = the XOR of f along the tree path from i to its anchor.
 *   Sign g     per component, from exact integer counts.  s_i is the dot below on the STORED N_i, negated iff x_i = 1.
 *              MVICP_ORIENT_ANCHOR: g = 0.  MVICP_ORIENT_VIEWPOINT: v = ref - p_i (per component), s_i = (N_i0 v0 + N_i1 v1) + N_i2 v2;
 *              g = 1 iff #(s_i < 0) > #(s_i > 0) over the component (a tie keeps the sign).  MVICP_ORIENT_DIRECTION: the same with v = ref.
 *              ref3 NULL = (0, 0, 0), legal for ANCHOR and VIEWPOINT only.
 *   Result     flip[i] = x_i XOR g_comp[i]; nrm[i] = N_i with every component negated iff flip[i] (a +0.0 becomes -0.0).
 * nrm is n x 3 doubles, flip n bytes, comp n ints, row i the ORIGINAL index i; n = 0 gives zero rows and 0 components.
 * The call performs mvicp_knn_search(frame, NULL, k, radius) internally and AFTERWARDS THAT SEARCH IS THE CONTEXT'S LAST NEIGHBOUR-SEARCH
 * RESULT, as with mvicp_fpfh.  Otherwise it is HISTORY-NEUTRAL, touches neither the frame's normals nor the estimate it read, needs the
 * frame's hash structure and NO graph; with several ranks every rank computes it locally.  The forest is built in Boruvka rounds on the
 * device; the host waits once per round (a round at least halves the number of trees that can still grow).  The result lives in
 * library-owned device memory of its own until the next mvicp_orient_normals, an upload to the same frame, mvicp_set_num_frames or
 * mvicp_destroy.  Profile scopes: those of the search, "orient_round", "orient_finish".
 * RETURNS THE NUMBER OF COMPONENTS (>= 0) or a negative mvicp_status.
 * Errors: NULL context, a frame index out of range, a source outside {0, 1}, k outside [2, 64], a mode outside mvicp_orient_mode, a
 * non-finite radius or ref entry, ref3 NULL with MVICP_ORIENT_DIRECTION -> MVICP_ERR_ARG, decided before the context is touched (earlier
 * results stay); a frame never uploaded, no normals of the asked source -> MVICP_ERR_STATE (earlier results stay). */
typedef enum { MVICP_ORIENT_ANCHOR = 0, MVICP_ORIENT_VIEWPOINT = 1, MVICP_ORIENT_DIRECTION = 2 } mvicp_orient_mode;
long long mvicp_orient_normals(mvicp_ctx* ctx, int frame, int source, int k, double radius, int mode, const double* ref3);
/* Copies the last result: nrm (n x 3 doubles), flip (n bytes), comp (n ints); each may be NULL; each may be a HOST pointer or a DEVICE
 * pointer of the context's device, decided per pointer as mvicp_voxel_fetch decides.  cap_rows = rows the destinations hold.
 * Errors: NULL context, cap_rows < n -> MVICP_ERR_ARG; no mvicp_orient_normals before -> MVICP_ERR_STATE. */
int mvicp_orient_fetch(mvicp_ctx* ctx, long long cap_rows, double* nrm, unsigned char* flip, int* comp);
/* The frame of the last mvicp_orient_normals takes that result's nrm as its normals: mvicp_normals_adopt with these values, same side
 * effects, same refusals (no result, or the frame was uploaded again since -> MVICP_ERR_STATE, with nothing changed). */
int mvicp_orient_adopt(mvicp_ctx* ctx);

/* Agreement between the normals of DIFFERENT clouds, over the correspondence lists the context holds (searched or explicit) at `poses`
 * (n_frames x 16).  Per owned edge e = (src, dst) and per pair (first, second) of its list: a = R_src N_first, b = R_dst N_second, each
 * component (r0 x + r1 y) + r2 z with the rows of the pose's rotation, t = (a0 b0 + a1 b1) + a2 b2, no fma; pos[e] counts t > 0, neg[e]
 * counts t < 0 (n_edges ints each; either may be NULL).  Edges of other ranks and edges whose source frame was fixed in the last
 * mvicp_correspond give 0 / 0.  HISTORY-NEUTRAL, one launch and one wait, integer sums (the counts are exact).  Profile scope
 * "normal_agreement".
 * Errors: NULL context or poses -> MVICP_ERR_ARG; what mvicp_linearize_metric(MVICP_METRIC_SYMMETRIC) refuses -- no graph, no list yet,
 * no normals on either frame of a non-empty list -> MVICP_ERR_STATE. */
int mvicp_normal_agreement(mvicp_ctx* ctx, const double* poses, int* pos, int* neg);
/* The sign rule on top of the counts (pure host function, no context; host pointers), in the style of mvicp_poses_from_pairs.  Edge e is
 * usable iff pos[e] + neg[e] >= min_count and pos[e] != neg[e].  The maximum spanning forest over the frames is the one Kruskal builds
 * from the usable edges in the order (|pos - neg| descending, e ascending).  component[f] = the lowest frame index of f's tree, which keeps
 * its sign; flip[f] = the XOR of [pos < neg] along the tree path from f to it.  component may be NULL.
 * RETURNS THE NUMBER OF COMPONENTS (>= 1).
 * Errors (MVICP_ERR_ARG): flip NULL, src / dst / pos / neg NULL with n_edges > 0, n_frames < 1, n_edges < 0, an edge index out of range or
 * src[e] == dst[e], a negative count, min_count < 0. */
int mvicp_signs_from_agreement(int n_frames, int n_edges, const int* src, const int* dst, const int* pos, const int* neg, int min_count,
                               unsigned char* flip, int* component);
/* Every stored normal of `frame` is negated, in original and in sorted order (a +0.0 becomes -0.0).  The side effects are exactly those of
 * mvicp_normals_adopt: owned lists that point into the frame are re-gathered, queued evaluations are voided.
 * Errors: NULL context, a frame index out of range -> MVICP_ERR_ARG; a frame never uploaded or without normals -> MVICP_ERR_STATE. */
int mvicp_negate_normals(mvicp_ctx* ctx, int frame);

/* ---- Descriptor matching and a consensus coarse pose, exactly specified -------------------------------------------------------
 * The stage that turns two sets of descriptors into a coarse pose: two device stages, one host rule between them.  Each result is a
 * pure function of the input bytes, bit for bit (tests/matchref.py is the same definition in numpy and as a scalar loop).  All
 * floating-point work is fp64, every operation rounded on its own, no fma; only + - x / sqrt and comparisons occur; comparisons are
 * IEEE as written, so NaN compares false.  Both device calls are HISTORY-NEUTRAL in the sense of
 * mvicp_knn_search, need NO graph and NO frame; with several ranks every rank computes locally.  Results live in library-owned device
 * memory until the next call of the same kind, mvicp_set_num_frames or mvicp_destroy.  Input and destination pointers may be HOST or
 * DEVICE pointers of the context's device, decided per pointer as mvicp_voxel_fetch decides (a device array must be fully written when
 * the call is made).  Argument errors are decided before the context is touched and leave earlier results alone.
 *
 * mvicp_feature_match: a has m rows, b has n rows, both row-major doubles with `dim` columns, 1 <= dim <= 64 (FPFH: 33), every value
 * finite, 0 <= m, n < 2^31.
 *   dist(a, b) s = +0.0; for c = 0 .. dim-1 in ascending order: t = a[c] - b[c]; s = s + t * t.  (a - b) and (b - a) are exact negatives,
 *              so dist is symmetric bit for bit.
 *   Forward    for each row i of a, the rows of b ordered by (dist, j): fwd_idx[i][0..1] and fwd_d2[i][0..1] are the first two entries;
 *              a missing entry is padded with idx -1 and d2 +inf.
 *   Backward   the same for each row j of b over the rows of a: bwd_idx (n x 2), bwd_d2 (n x 2).
 * Option "match_chunk" (default 2048) sets the rows of the other operand per chunk of the brute-force kernel; it changes the speed only,
 * the result is the same bytes.  Profile scopes: "match_fwd", "match_bwd", "match_merge".
 * RETURNS m (>= 0; m = 0 or n = 0 is not an error) or a negative mvicp_status.
 * Errors: NULL context, dim outside [1, 64], m or n outside [0, 2^31), a NULL operand with rows -> MVICP_ERR_ARG; a non-finite descriptor
 * value -> MVICP_ERR_ARG, reported by this call, and no result is left behind. */
long long mvicp_feature_match(mvicp_ctx* ctx, const double* a, long long m, const double* b, long long n, int dim);
/* Copies the last result: fwd_idx (m x 2 ints), fwd_d2 (m x 2 doubles), bwd_idx (n x 2 ints), bwd_d2 (n x 2 doubles); each may be NULL.
 * cap_m / cap_n = rows the forward / backward destinations hold.
 * Errors: NULL context, cap_m < m, cap_n < n -> MVICP_ERR_ARG; no mvicp_feature_match before -> MVICP_ERR_STATE. */
int mvicp_feature_match_fetch(mvicp_ctx* ctx, long long cap_m, long long cap_n, int* fwd_idx, double* fwd_d2, int* bwd_idx, double* bwd_d2);

/* The pair rule on top of the fetched arrays (pure host function, no context; host pointers).  Pair (i, j = fwd_idx[i][0]) is kept iff
 *   j >= 0;  mutual == 0 or bwd_idx[j][0] == i;  ratio >= 1 (ratio test off) or fwd_d2[i][0] <= (ratio * ratio) * fwd_d2[i][1].
 * Pairs are written to `pairs` (room for m x 2 ints) as (i, j) in ascending i.  RETURNS THE NUMBER OF PAIRS (>= 0).
 * Errors: a NULL pointer, m or n < 0, a ratio that is NaN or <= 0, an index j >= n -> MVICP_ERR_ARG. */
long long mvicp_match_pairs(long long m, long long n, const int* fwd_idx, const double* fwd_d2, const int* bwd_idx, int mutual, double ratio,
                            int* pairs);

/* mvicp_consensus: p, q are n_pairs x 3 doubles, index-aligned pairs from source to destination, all finite, 3 <= n_pairs < 2^31;
 * 1 <= hypotheses <= 2^24; tau > 0; edge_sim s in [0, 1) (s = 0 makes the edge check vacuous).  With c = n_pairs:
 *   Forms      dot (x0 y0 + x1 y1) + x2 y2; cross componentwise x1 y2 - x2 y1, ...; a row times a vector (r0 v0 + r1 v1) + r2 v2.
 *   Sample     hypothesis h, slot t in {0, 1, 2}: z = seed + (3 h + t + 1) * 0x9E3779B97F4A7C15 (mod 2^64);
 *              z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; u = z ^ (z >> 31);
 *              index = ((u >> 32) * c) >> 32.  Rejected if two of the three indices are equal.
 *   Edges      s2 = s * s; for each of the edges (0,1), (1,2), (2,0): lp = dot(p_a - p_b, p_a - p_b), lq likewise; both
 *              lp >= s2 * lq and lq >= s2 * lp are needed, rejected otherwise.
 *   Frame      u1 = p1 - p0, n1 = sqrt(dot(u1, u1)), rejected if n1 == 0, e1 = u1 / n1; w = cross(e1, p2 - p0), nw = sqrt(dot(w, w)),
 *              rejected if nw == 0, e3 = w / nw; e2 = cross(e3, e1); f1, f2, f3 from the q triangle in the same way.
 *   Pose       R[r][k] = (f1[r] e1[k] + f2[r] e2[k]) + f3[r] e3[k]; cp = ((p0 + p1) + p2) / 3.0 and cq likewise; t = cq - R cp.
 *   Score      tau2 = tau * tau; pair i is an inlier iff dot(r, r) <= tau2 with r = (R p_i + t) - q_i; count[h] = the number of inliers,
 *              or -1 for a rejected hypothesis.
 *   Winner     the largest count, the lowest h among equals.
 * *result: best = the winner's index (-1 when nothing was accepted), count = its count, accepted = the number of accepted hypotheses,
 * pose = 16 column-major doubles.  When every hypothesis is rejected best = -1, count = 0, the pose is the identity and no flag is set;
 * that is not an error.  Profile scopes: "cons_hyp", "cons_score", "cons_pick".
 * RETURNS MVICP_OK or a negative mvicp_status.
 * Errors: NULL context or pointer, n_pairs < 3 or >= 2^31, hypotheses outside [1, 2^24], a tau that is not finite or <= 0, an edge_sim
 * outside [0, 1) -> MVICP_ERR_ARG; a non-finite coordinate -> MVICP_ERR_ARG, reported by this call, and no result is left behind. */
typedef struct mvicp_consensus_result {
  int best, count, accepted, reserved;
  double pose[16];
} mvicp_consensus_result;
int mvicp_consensus(mvicp_ctx* ctx, const double* p, const double* q, long long n_pairs, long long hypotheses, unsigned long long seed,
                    double tau, double edge_sim, mvicp_consensus_result* result);
/* Copies the last result: count (hypotheses ints), flags (n_pairs bytes: 1 = an inlier of the winner); each may be NULL.
 * Errors: NULL context, cap_h < hypotheses, cap_c < n_pairs -> MVICP_ERR_ARG; no mvicp_consensus before -> MVICP_ERR_STATE. */
int mvicp_consensus_fetch(mvicp_ctx* ctx, long long cap_h, int* count, long long cap_c, unsigned char* flags);

/* ---- Batched coarse poses over an edge list, and initial poses from them ---------------------------------------------------------
 * mvicp_coarse_pairs: desc (total x dim doubles) and xyz (total x 3 doubles) are the concatenated descriptors and points of n_sets
 * sets; set s owns rows offsets[s] .. offsets[s+1] (offsets: n_sets + 1 non-decreasing host values starting at 0; empty sets are
 * allowed).  desc, xyz and the fetch destinations may each be a HOST or a DEVICE pointer, decided per pointer as mvicp_voxel_fetch
 * decides; offsets, src, dst, seeds and results are host pointers.
 * CONTRACT, by reduction: for edge e with a = src[e], b = dst[e], m_a and m_b their rows, results[e] and the fetched arrays equal, byte
 * for byte, the chain
 *   1  mvicp_feature_match(desc_a, m_a, desc_b, m_b, dim)
 *   2  mvicp_match_pairs(..., mutual, ratio): c pairs in ascending i
 *   3  P = xyz_a[pairs[:,0]], Q = xyz_b[pairs[:,1]]
 *   4  mvicp_consensus(P, Q, c, hypotheses, seeds[e], tau, edge_sim) when c >= 3; otherwise best = -1, count = 0, accepted = 0, the
 *      identity pose and no flag set.
 * results[e].pairs = c.  Each distinct ordered set pair is matched once, whatever the edge list repeats or reverses.  Option
 * "match_chunk" changes the speed only.  HISTORY-NEUTRAL, needs NO graph and NO frame; the result lives in storage of its own (the last
 * results of mvicp_feature_match, mvicp_consensus, mvicp_fpfh and mvicp_knn_search are left untouched) until the next mvicp_coarse_pairs,
 * mvicp_set_num_frames or mvicp_destroy; a failed call leaves none behind.  The host waits for the device twice per call, however many
 * edges.  Profile scopes: "coarse_match", "coarse_merge", "coarse_rule", "coarse_hyp", "coarse_score", "coarse_pick".
 * RETURNS n_edges (n_edges = 0 is not an error) or a negative mvicp_status.
 * Errors (MVICP_ERR_ARG, decided before the context is touched): NULL context or pointer, dim outside [1, 64], n_sets < 1, n_edges
 * outside [0, 65535], an edge index out of range or src[e] == dst[e], offsets that do not start at 0 or decrease, a total >= 2^31,
 * hypotheses outside [1, 2^24], n_edges x hypotheses > 2^28, a ratio that is NaN or <= 0, a tau that is not finite or <= 0, an edge_sim
 * outside [0, 1); a non-finite descriptor or coordinate -> MVICP_ERR_ARG, reported by this call, and no result is left behind. */
typedef struct mvicp_coarse_edge {
  int pairs, best, count, accepted;
  double pose[16];
} mvicp_coarse_edge;
long long mvicp_coarse_pairs(mvicp_ctx* ctx, const double* desc, const double* xyz, const long long* offsets, int n_sets, int dim, int n_edges,
                             const int* src, const int* dst, const unsigned long long* seeds, int mutual, double ratio, long long hypotheses,
                             double tau, double edge_sim, mvicp_coarse_edge* results);
/* Copies edge `edge` of the last result: pairs (c x 2 ints, (i, j) in ascending i), flags (c bytes: 1 = an inlier of the winner); each
 * may be NULL.  cap_pairs = pairs the destinations hold.
 * Errors: NULL context, an edge out of range, cap_pairs < c -> MVICP_ERR_ARG; no mvicp_coarse_pairs before -> MVICP_ERR_STATE. */
int mvicp_coarse_pairs_fetch(mvicp_ctx* ctx, int edge, long long cap_pairs, int* pairs, unsigned char* flags);

/* Initial poses from pairwise poses (pure host function, no context; host pointers).  pose[e] (16 column-major doubles) maps coordinates
 * of frame src[e] into those of frame dst[e], as mvicp_consensus returns it; the poses written map frame to world.  Edge e is usable
 * iff count[e] >= min_count.
 *   Rule         a maximum spanning forest, Prim, deterministic: the reached set starts as {root}; among the usable edges with exactly
 *                one endpoint reached take the largest count, the lowest e among equals; repeat until none is left.  If frames remain,
 *                the lowest unreached index starts the next component: its pose is the identity, its parent and parent_edge -1.
 *                component[i] numbers the components in the order they start (the root's is 0).  More than one component is reported,
 *                not repaired.
 *   Composition  fp64, every operation rounded on its own, no fma.  With T = pose[e]: the new frame is dst[e]: pose_child = pose_parent
 *                T^-1, T^-1 = [R^T | -(R^T t)]; the new frame is src[e]: pose_child = pose_parent T.  A product has R = Ra Rb, each
 *                entry (a0 b0 + a1 b1) + a2 b2, t = (Ra tb) + ta with a row times a vector as (r0 v0 + r1 v1) + r2 v2, and the bottom
 *                row 0 0 0 1.  The root's pose is root_pose as given (NULL: the identity).
 * parent, parent_edge and component may be NULL.  RETURNS THE NUMBER OF COMPONENTS (>= 1).
 * Errors (MVICP_ERR_ARG): poses_out NULL, src / dst / count / pose NULL with n_edges > 0, n_frames < 1, n_edges < 0, root out of range,
 * an edge index out of range or src[e] == dst[e], min_count < 0. */
int mvicp_poses_from_pairs(int n_frames, int n_edges, const int* src, const int* dst, const int* count, const double* pose, int min_count,
                           int root, const double* root_pose, double* poses_out, int* parent, int* parent_edge, int* component);

/* The rounding allowance of the temporal cache (pure host function, no context): what mvicp_correspond adds to the displacement |dM p + dv|
 * of an edge's queries between the search at (pose_src_old, pose_dst_old) and the one at (pose_src, pose_dst), poses as 16 column-major
 * doubles, max_norm >= max |p| over the source cloud.  With x = (Rs, ts, Rd^-1, td) the query transform of a pose pair (Rd^-1 as
 * mvicp_correspond computes it) and B(x) = ||Rd^-1||_F (|ts| + 16 ||Rs||_F max_norm + 13 |ts - td|):
 *   *out = 2^-52 (B(x_old) + B(x_new)), and 0 iff the two transforms are bit-identical (then every query is, too).
 * It bounds the rounding of both evaluations of the fp64 query map (which rounds R p + ts at the size of ts, not of ts - td) and of
 * dM, dv themselves; the derivation is at cache_allowance_xf in csrc/search_plan.h and in DESIGN.md section 3.4.
 * Errors: a NULL pointer, max_norm < 0 or NaN -> MVICP_ERR_ARG. */
int mvicp_cache_allowance(const double* pose_src_old, const double* pose_dst_old, const double* pose_src, const double* pose_dst,
                          double max_norm, double* out);

/* The graph rule on top of the census (pure host function, no context).  Frame i keeps the knn frames j != i with the most hits, among
 * those with hits[i*K+j] > 0 and hits[i*K+j] >= min_fraction * samples[i]; equal hits: the smaller sumq first (within one row that is
 * the smaller mean distance: an exact integer comparison, no division), then the lower j.  sumq NULL: hits, then lower j.  Edges are
 * written src ascending, neighbours best first (the reference's order, main_multiview.cpp:104-117); skip_frame0 != 0 omits the edges
 * OUT OF frame 0 (never searched: frame.cpp:93).  *n_components (may be NULL) = connected components of the undirected graph over all
 * K frames, edges out of frame 0 included whether or not they are written.  A graph with more than one component is reported, not
 * repaired.  RETURNS THE NUMBER OF EDGES (>= 0); more than cap is MVICP_ERR_ARG. */
int mvicp_graph_from_overlap(int n_frames, const int* samples, const int* hits, const long long* sumq, int knn, double min_fraction,
                             int skip_frame0, int cap, int* src, int* dst, int* n_components);

/* Multi-GPU: this rank owns a contiguous chunk of the edge list (balanced by N_src).  Call before
 * mvicp_set_graph.  Default rank 0 of 1.  Non-OK returns: world < 1 or rank outside [0, world) -> MVICP_ERR_ARG; called while a
 * graph exists -> MVICP_ERR_STATE; rank and world stay what they were. */
int mvicp_set_shard(mvicp_ctx* ctx, int rank, int world);
/* The partition rule itself (pure host function, no context): owner[e] in [0, world) for edges with n_src[e]
 * source points each.  Contiguous chunks, balanced by source points. */
int mvicp_edge_owner(int n_edges, const int* n_src, int world, int* owner);
/* RCCL communicator for the per-edge normal-equation all-reduce.  librccl_path: the librccl.so to
 * dlopen (pass the one torch already loaded, or NULL for "librccl.so.1").  unique_id: 128 bytes
 * produced by mvicp_comm_unique_id on rank 0 and broadcast by the launcher. */
int mvicp_comm_unique_id(const char* librccl_path, void* unique_id_128);
int mvicp_comm_init(mvicp_ctx* ctx, const char* librccl_path, const void* unique_id_128, int rank, int world);
/* Ranks of the communicator as RCCL itself reports them (ncclCommCount): 0 = no communicator, -1 = this librccl does not say. */
int mvicp_comm_nranks(mvicp_ctx* ctx);

/* Alternative exchange without RCCL: the launcher supplies an in-place sum all-reduce over HOST doubles (e.g. MPI or
 * torch.distributed/gloo); the library stages the per-edge blocks through host memory.  Same sharding, same exactness;
 * meant for bring-up and for testing the N > 1 path where RCCL cannot run (several ranks on one GPU). */
typedef int (*mvicp_allreduce_fn)(void* user, double* host_buf, size_t n);
int mvicp_comm_set_callback(mvicp_ctx* ctx, mvicp_allreduce_fn fn, void* user);

/* ---- S1: correspondence search ----------------------------------------------------------------
 * Replaces, for ALL non-fixed frames at once, Frame::computeClosestPointsToNeighbours(frames, thresh)
 * (include/frame.h:54, src/internal/frame.cpp:91-185; caller main_multiview.cpp:119-127).
 *   poses  : n_frames x 16;  fixed : n_frames bytes (edges whose src is fixed are skipped, frame.cpp:93)
 *   thresh : the float cutoff (frame.h:54)
 *   counts / weights (n_edges, may be NULL): |correspondances| and OutgoingEdge::weight =
 *            (float)(1.5 * upper median distance) (frame.cpp:166-176).  weight of an empty edge = 0. */
int mvicp_correspond(mvicp_ctx* ctx, const double* poses, const unsigned char* fixed, float thresh, int nn_method,
                     int* counts, float* weights);
/* Start a new registration on the same clouds and graph: forget everything earlier searches left behind (temporal NN cache, seeds,
 * reusable lists, settled medians, MVICP_NN_AUTO state, the queued evaluation).  The next mvicp_correspond behaves like the first one
 * after mvicp_set_graph — the state of a fresh run of the reference program (main_multiview.cpp:130-148).  Host-only bookkeeping. */
int mvicp_reset_history(mvicp_ctx* ctx);
/* Copy edge e's list back as Frame::neighbours[j].correspondances (frame.h:18-22): ascending `first`.
 * RETURNS THE NUMBER OF TRIPLES WRITTEN (>= 0, = counts[e] of the last mvicp_correspond) or a negative mvicp_status;
 * cap is the capacity of the three output arrays (each may be NULL to skip that field).
 * Non-OK returns (this call and mvicp_map_correspondences): an edge out of range, cap < count, a NULL output -> MVICP_ERR_ARG; no list
 * yet, an edge of another rank -> MVICP_ERR_STATE.  Nothing changes. */
int mvicp_get_correspondences(mvicp_ctx* ctx, int edge, int cap, int* first, int* second, double* dist);
/* ALL lists of the last mvicp_correspond at once, as the reference lays them out: `struct Correspondance {int first; int second; double
 * dist;}` (include/frame.h:18-22), ascending `first` within an edge (frame.cpp:129,156-160).  One device pass un-sorts every edge this
 * rank owns, ONE asynchronous copy brings the triples into pinned host memory OWNED BY THE LIBRARY:
 *   *triples            -> the buffer;   *offsets -> n_edges + 1 positions: edge e = (*triples)[(*offsets)[e] .. (*offsets)[e + 1])
 * (zero width for edges of other ranks, edges whose source is fixed and edges that hold an explicit list).  Both pointers stay valid until
 * the next mvicp_correspond that changes a list (see mvicp_correspondence_epochs) / mvicp_set_correspondences / mvicp_set_graph /
 * mvicp_reset_history / mvicp_destroy on this context.  The
 * first call after a search does the work, later calls (and mvicp_get_correspondences, which slices the same buffer) are free. */
typedef struct mvicp_corr { int first; int second; double dist; } mvicp_corr;
int mvicp_map_correspondences(mvicp_ctx* ctx, const mvicp_corr** triples, const long long** offsets);
/* The same export WITHOUT waiting for it: the device pass is queued and the triples travel to the pinned buffer in chunks (one per run of edges with
 * the same source frame, in edge order).  *triples / *offsets are valid at once (the offsets are known from the search's counts); the BYTES of edge e
 * may be read after mvicp_wait_correspondences(ctx, e) returned — which waits for e's chunk only, so a caller that fills Frame::neighbours frame by
 * frame (frame.cpp:91-185 is called once per frame, main_multiview.cpp:119-127) copies frame i while the lists of frames i + 1 .. are still on the
 * bus.  Any later library call that waits for the stream (mvicp_map_correspondences, mvicp_get_correspondences, mvicp_optimize ...) completes it too. */
int mvicp_map_correspondences_async(mvicp_ctx* ctx, const mvicp_corr** triples, const long long** offsets);
int mvicp_wait_correspondences(mvicp_ctx* ctx, int edge);
/* Per-edge change counters of the lists, for callers that keep their own copy (the Frame mirror's `neighbours[j].correspondances`,
 * frame.cpp:110,156-160: the reference clears and refills every list every round; a caller that holds edge e's list with epoch x may skip the
 * refill while (*epochs)[e] == x).  An edge keeps its epoch across an mvicp_correspond iff its list is PROVABLY last search's bit for bit — same
 * cutoff, both poses bit-identical, searched then and now (a search is a pure function of these) — e.g. every edge in the rounds after the
 * registration has converged; then mvicp_map_correspondences returns the buffer it already holds without any device work.  Every other event
 * (a search with different inputs, mvicp_set_correspondences, mvicp_reset_history, a change of the "tie_rule" option, a failed search — ANY
 * mvicp_correspond that does not return MVICP_OK drops the whole cross-round state, as mvicp_reset_history does) gives the edge a new, never repeated epoch.
 * *epochs -> n_edges counters owned by the library, valid until mvicp_set_graph / mvicp_destroy. */
int mvicp_correspondence_epochs(mvicp_ctx* ctx, const unsigned long long** epochs);
/* Install an explicit list (pairwise known-correspondence case, main_pairwise.cpp:60-61; tests).
 * Non-OK returns: an edge out of range, n < 0 or n > N_src, NULL lists with n > 0, an index out of range anywhere in the lists ->
 * MVICP_ERR_ARG; an edge of another rank -> MVICP_ERR_STATE.  The whole list is checked before the edge is touched: the edge keeps the
 * list it had (searched or explicit), its epoch and its weight. */
int mvicp_set_correspondences(mvicp_ctx* ctx, int edge, int n, const int* first, const int* second, float weight);

/* S1': batch form of Frame::getClosestPoint (frame.h:55, frame.cpp:187-206): queries are already in
 * the frame's local coordinates; returns index and SQUARED distance per query.
 * Non-OK returns: a frame out of range, n < 0, a NULL buffer with n > 0, an nn_method outside mvicp_nn_method -> MVICP_ERR_ARG, decided
 * before anything is allocated or built; an empty frame, a failed structure build -> MVICP_ERR_STATE.  The call never changes a frame. */
int mvicp_nn_query(mvicp_ctx* ctx, int frame, const double* queries, int n, int nn_method, int* idx, double* d2);

/* ---- normal equations ---------------------------------------------------------------------------
 * Per edge: the 12x12 Gauss-Newton block of  sum rho(||r||^2)/2  in canonical right-perturbation
 * coordinates [upsilon_s, omega_s, upsilon_d, omega_d]  (T <- T exp(delta)), i.e. what
 * Ceres accumulates from the residual blocks of include/icp-ceres.h:49-316 + SoftLOneLoss(edge.weight)
 * (icp-ceres.cpp:284,374,449).  out: n_edges x 91 = [78 upper-triangular row-major H | 12 g | cost]. */
#define MVICP_EDGE_BLOCK 91
/* Non-OK returns of both evaluations (and of mvicp_optimize, which evaluates): a NULL pointer -> MVICP_ERR_ARG; no graph, no list yet
 * (neither mvicp_correspond nor mvicp_set_correspondences), point-to-plane while the target of a non-empty list has no normals ("...
 * needs normals on frame i") -> MVICP_ERR_STATE.  Lists, epochs and poses are untouched; `out` is not written.
 * With several ranks (an exchange configured) a refusal is a verdict on the lists THIS rank owns, and it is the same call on every rank that
 * returns non-OK: a rank that refuses ("no list yet", "... needs normals on frame i") still enters the evaluation's one collective, with the
 * exchanged buffer poisoned, and returns its own MVICP_ERR_STATE; every other rank returns MVICP_ERR_COMM ("a peer rank failed ...") from
 * the same call — the protocol of a failed local launch.  No rank is left waiting in the all-reduce, no rank gets blocks, and the next
 * evaluation (after mvicp_recompute_normals on that frame on every rank, say) is an ordinary one.  After a search the counts are global,
 * but the verdict is still taken from the owned edges only: after mvicp_set_correspondences only the owner knows an edge's count (the other
 * ranks keep the last search's), and a rule that every rank decides from its own copy would let them disagree.  What the caller owes on a
 * sharded context with explicit lists: every rank makes the same sequence of evaluation calls; every rank holds lists before the first of
 * them (a search, or mvicp_set_correspondences for each edge it owns that is to be non-empty — a rank that has neither refuses, and with it
 * every rank); and, because mvicp_set_correspondences drops the evaluation a search queued ahead on the calling rank only, explicit lists are
 * not mixed with queued evaluations: set "spec_eval" 0 on every rank of a sharded context that installs explicit lists between searches. */
int mvicp_linearize(mvicp_ctx* ctx, const double* poses, int point_to_plane, int robust, double* out);
/* Two evaluations on the SAME correspondences and scales: out_a = what mvicp_linearize gives at poses_a, out_b = what it gives at poses_b,
 * bit for bit.  On a single rank both come from one kernel that reads the operand stream once (the kernel is bandwidth-bound, so the pair
 * costs little more than one evaluation); with an exchange configured (N > 1 ranks) it is two ordinary evaluations.  The single-rank path does
 * not touch the evaluations mvicp_correspond queued ahead, nor their buffers.  Profile scope: "linearize_pair". */
int mvicp_linearize_pair(mvicp_ctx* ctx, const double* poses_a, const double* poses_b, int point_to_plane, int robust, double* out_a, double* out_b);

/* The objective by name.  POINT and PLANE are the reference's two (mvicp_linearize with point_to_plane 0 / 1; any non-zero flag there is
 * PLANE).  SYMMETRIC is the symmetric point-to-plane objective (Rusinkiewicz, SIGGRAPH 2019): with p~ the source point in the dst frame
 * and nu the source normal rotated into it,
 *     r = m . (p~ - q),  m = (n_q + nu) / 2,
 * the residual along the MEAN of the two normals: zero at the true pose wherever the surface is locally quadratic between the two
 * samples, where the point-to-plane residual n_q . (p~ - q) keeps a curvature bias.  The factor 1/2 makes r the point-to-plane residual
 * when the two normals agree, so the loss, the scale a = edge.weight and the cost sum rho / 2 are those of PLANE.  Per row
 * u = [m ; (p~ x n_q + q x nu) / 2], J = [Ad^T u ; -u] in the coordinates above (csrc/linearize_sym.hip).
 * THE NORMALS ARE USED AS STORED: no sign flip, no normalisation.  Orienting the normals of the clouds consistently with each other
 * (the same side of the surface in every frame) is the caller's job -- mvicp_estimate_normals with each view's sensor position as
 * viewpoint is the tool for it, mvicp_orient_normals + mvicp_normal_agreement + mvicp_signs_from_agreement + mvicp_negate_normals where
 * there is no sensor position; with opposite orientations m is half the DIFFERENCE of the normals.
 * The source normal is the source frame's current one: after mvicp_recompute_normals the next evaluation sees the new normals.
 * For this objective the relative transform of an edge is formed with the true inverse of the destination's rotation, in extended
 * precision (for a rotation that is its transpose): the result does not depend on how far the given poses are from orthonormal to the
 * last bit.  (A destination matrix that is no rotation at all, determinant outside (0.5, 2), gets the transpose like the other objectives:
 * finite values, meaningless blocks.)  Accuracy contract: tests/test_gpu_sym_accuracy.py (32 x a plain fp64 evaluation's error against a long-double reference). */
typedef enum { MVICP_METRIC_POINT = 0, MVICP_METRIC_PLANE = 1, MVICP_METRIC_SYMMETRIC = 2 } mvicp_metric;
/* mvicp_linearize with the objective named.  Metric 0 / 1 ARE mvicp_linearize(point_to_plane = 0 / 1): same code path, same bytes, the
 * same use of the evaluations mvicp_correspond queued ahead.  SYMMETRIC always takes the ordinary route (relative transforms and scales
 * uploaded, one launch, the all-reduce when an exchange is configured, one wait; profile scope "linearize_sym") and is never queued or
 * paired.  Non-OK returns as mvicp_linearize, and: a metric outside mvicp_metric -> MVICP_ERR_ARG; SYMMETRIC while the destination OR the
 * source of a non-empty list has no normals ("symmetric needs normals on frame i") -> MVICP_ERR_STATE. */
int mvicp_linearize_metric(mvicp_ctx* ctx, const double* poses, int metric, int robust, double* out);

/* The plane-to-plane objective: Generalized-ICP (Segal, Haehnel, Thrun, RSS 2009) in its standard form, where the covariance of a point is a
 * function of its normal alone, C(n) = I - (1 - epsilon) n^ n^T: epsilon along the normal, 1 in the tangent plane.  Per correspondence, with
 * the relative transform (A, t) of the edge formed as for SYMMETRIC (the true inverse of R_d in extended precision, hi + lo parts):
 *     p~ = A p + t,   f = p~ - q,   nu = A n_p
 *     P(n) = n n^T / (n . n)  if 2^-1022 <= n . n < inf (as computed in fp64),  else the zero matrix       (such a normal means C = I)
 *            (n . n zero, subnormal, overflowed or NaN: a zero normal, one with a NaN or Inf component, one whose components are below
 *             about 1e-154 or above about 1e154 in size.  A subnormal n . n has lost the bits that say how long n is.)
 *     S = 2 I - (1 - epsilon) (P(n_q) + P(nu)),      W = 2 epsilon S^-1                  (symmetric, eigenvalues in [epsilon, 1])
 *     s = f^T W f
 *     J_f = [ A , -A [p]x , -I , [p~]x ]                                  (3 x 12, coordinates [ups_s om_s ups_d om_d], T <- T exp(delta))
 *     H = sum w J_f^T W J_f,   g = sum w J_f^T W f,   cost = sum rho(s) / 2
 * The loss, the corrector weight w, the scale a = edge.weight and the cost are those of POINT: soft-L1 on the squared length of a three-vector.
 * W IS FROZEN: it is held at its value at the evaluation poses, fixed in the destination frame, while f is differentiated — the Gauss-Newton
 * form of Segal's section III, of PCL and of Open3D; the term with dW / d(pose) is dropped.  The cost returned at candidate poses uses W at those
 * poses.  The factor 2 epsilon makes the largest weight 1, so s <= |f|^2 and the robust scale keeps its meaning.  epsilon = 1 is POINT's
 * objective (W = I: the same cost and the same g; H differs from POINT's in the om_d blocks by terms of first order in f, because f is the
 * residual in the destination frame, whose om_d rows are [p~]x where POINT's are [q]x).  With agreeing unit normals
 * W = epsilon I + (1 - epsilon) n n^T: PLANE in the limit epsilon -> 0.
 * THE NORMALS ARE USED AS STORED, and P(n) depends on neither the sign nor the length of n: their orientation does not matter for this
 * objective.  The source normal is the source frame's current one (after mvicp_recompute_normals the next evaluation sees the new normals).
 * epsilon must be finite and within [1e-6, 1]; anything else -> MVICP_ERR_ARG.
 * The evaluation takes the ordinary route (relative transforms and scales uploaded, one launch, the all-reduce when an exchange is configured,
 * one wait; profile scope "linearize_gicp") and is never queued or paired.  Non-OK returns as mvicp_linearize, and: while the destination OR
 * the source of a non-empty list has no normals ("gicp needs normals on frame i") -> MVICP_ERR_STATE.  A refused call changes nothing.
 * Accuracy contract: the symmetric objective's — per piece at most 32 x the error of a plain fp64 evaluation of the direct rows against a
 * long-double reference (tests/test_gpu_gicp_accuracy.py, tests/gicpref.py).  Kernel: csrc/linearize_gicp.hip.
 * This objective has NO mvicp_metric value: the metric calls refuse 3 as before. */
int mvicp_linearize_gicp(mvicp_ctx* ctx, const double* poses, double epsilon, int robust, double* out);

/* ---- S2: the LM solve ----------------------------------------------------------------------------
 * Replaces ICP_Ceres::ceresOptimizer / _ceresAngleAxis / _sophusSE3 (frames, pointToPlane, robust)
 * (include/icp-ceres.h:40-42; caller main_multiview.cpp:158-161).  poses in/out (frames[i]->pose).
 * fixed[0] is forced to 1 like icp-ceres.cpp:244,341,417.  Edges whose SOURCE frame is fixed contribute nothing (no cost, no
 * normal-equation terms), whatever correspondences they hold: the reference adds no residual blocks for them
 * (`if(srcCloud.fixed) continue;` icp-ceres.cpp:255,351,426).  An edge with a fixed DESTINATION keeps its residuals. */
typedef struct mvicp_summary {
  double initial_cost, final_cost;
  int iterations;        /* LM iterations after the initial evaluation (<= max_iterations) */
  int successful_steps;
  int termination;       /* 0 max-iterations, 1 gradient tol, 2 parameter tol, 3 function tol, 4 radius, -1 failure */
  int evaluations;       /* device linearize launches */
} mvicp_summary;
/* One deliberate deviation from the reference's write-back (icp-ceres.cpp:312-321,386-394,472-474 always converts the parameter
 * blocks back to poses, which re-orthonormalises R): a solve that ends WITHOUT taking a step (successful_steps == 0) returns the
 * caller's poses bit for bit.  pose -> parameters -> pose is a last-bit 2-cycle for some rotations, and the round trip would keep a
 * converged registration from being a fixed point of the round.  Costs in the summary are those of the round-tripped poses the
 * solver evaluates at (they differ from the returned ones by that last bit at most).  Callers that hand in a NON-orthonormal
 * rotation and rely on the write-back to repair it must orthonormalise it themselves. */
/* Non-OK returns: a param outside mvicp_param -> MVICP_ERR_ARG; what mvicp_linearize refuses -> MVICP_ERR_STATE; `poses` come back as
 * they were passed.  A step the trust region REJECTS is not an error: iterations counts it, successful_steps does not, and the solve goes
 * on from the kept normal equations with a smaller radius (tests/test_gpu_lm_rejected.py). */
int mvicp_optimize(mvicp_ctx* ctx, double* poses, unsigned char* fixed, int param, int point_to_plane, int robust,
                   int max_iterations /* reference: 50, icp-ceres.cpp:81 */, mvicp_summary* summary);
/* mvicp_optimize with the objective named (mvicp_metric above).  Metric 0 / 1 ARE mvicp_optimize(point_to_plane = 0 / 1), including the
 * arming of the evaluations the next mvicp_correspond queues ahead.  A SYMMETRIC solve arms nothing and voids what is queued, as a failed
 * solve does: the search after it queues no evaluation.  A metric outside mvicp_metric -> MVICP_ERR_ARG. */
int mvicp_optimize_metric(mvicp_ctx* ctx, double* poses, unsigned char* fixed, int param, int metric, int robust,
                          int max_iterations, mvicp_summary* summary);
/* mvicp_optimize over the plane-to-plane objective (mvicp_linearize_gicp above; epsilon within [1e-6, 1], else MVICP_ERR_ARG).  Like a
 * SYMMETRIC solve it arms nothing and voids what is queued: the search after it queues no evaluation. */
int mvicp_optimize_gicp(mvicp_ctx* ctx, double* poses, unsigned char* fixed, int param, double epsilon, int robust,
                        int max_iterations, mvicp_summary* summary);

/* Host-only form of the same solver over a caller-supplied evaluator (no GPU touched by this call):
 * eval(user, poses[n_frames x 16], blocks[n_edges x 91]) must fill the per-edge canonical blocks exactly
 * as mvicp_linearize does.  mvicp_optimize is this with the device evaluator plugged in.
 * With MVICP_LM_TRACE set in the environment every solve (this one and mvicp_optimize's) writes one line per iteration that evaluated a
 * candidate to stderr: "[mvicp lm] it I cost C cand C' radius R model_change M" — the accept / reject decision is (C - C') / M against 1e-3. */
typedef int (*mvicp_eval_fn)(void* user, const double* poses, double* blocks);
int mvicp_lm_solve(int n_frames, int n_edges, const int* src, const int* dst, double* poses, unsigned char* fixed, int param,
                   int max_iterations, mvicp_eval_fn eval, void* user, mvicp_summary* summary);

/* ---- closed-form pairwise solvers (host only; no GPU touched) ----------------------------------------
 * Replace ICP_Closedform::pointToPoint / pointToPlane (include/icp-closedform.h:10-11, src/internal/icp-closedform.cpp:9-26,
 * 30-54): the reference's comparison baselines in main_pairwise.cpp:74-76,93-95 and an independent check of the
 * point-to-point / point-to-plane normal equations.  Index-aligned pairs (src[i], dst[i]) (and nor[i], the normal at dst[i]);
 * pose_out = the src -> dst transform, 16 doubles column-major.  point_to_point: the least-squares rigid transform (exact);
 * point_to_plane: one linearised step from identity with R = Rx Ry Rz of the three solved angles (icp-closedform.cpp:47-51). */
int mvicp_closedform_point_to_point(const double* src, const double* dst, int n, double* pose_out);
int mvicp_closedform_point_to_plane(const double* src, const double* dst, const double* nor, int n, double* pose_out);

/* Tuning / test switches.  "nn_tree_only" (0/1): skip the hash-grid fast path and answer every query with the
 * exact AABB-tree descent (same results; used by the parity tests to exercise the fallback on every query).
 * "grid_target" (points per occupied hash cell the cell-edge heuristic aims at; set before mvicp_set_frame).
 * "nn_cache" (0/1, default 1): temporal cache of the grid kernel — a query whose previous neighbour is provably still
 * nearest after the pose update skips the search (results are bit-identical either way).
 * "nn_census" (0/1): count candidates / boxes / cache hits per launch while profiling (feeds the algorithmic-byte model).
 * "voxel_permute" (0/1, default 1): mvicp_voxel_grid lays the transformed points out in sorted order before it sums them (0: the
 * sum re-gathers them through the sorted sequence; the result is the same bytes).
 * "spin_wait" (0/1, default 0): poll the stream for up to 2 ms before blocking on the per-evaluation / per-round waits.
 * "tile_seed" (0/1, default 1): the tile kernel starts from last round's neighbours; "tile_waves" (0 = auto, 4..8):
 * occupancy variant of the tile kernel; "tile_mfma" (0/1/2, default 1): the tile method screens an opened tile on the matrix pipe
 * (nn_mfma_kernel) — 1: except in cache-aware rounds, 2: always, 0: never (the fp32 VALU screen of nn_tile_kernel); "mfma_kacc" (default
 * 34): allowance for the fp32 accumulation inside one matrix instruction, in units of 2^-24 x sum |terms| (34 = seventeen truncating
 * additions; lower values are a measured, not a proven, bound); "mfma_trig" (default 2): a lane with more screen hits than this in one
 * tile makes the wave confirm nearest-first and screen the tile again; "mfma_lbt" (0/1, default 1): launches without any seed test a tile's box per
 * lane before screening it; "nn_search_factor" (default 4; 0 = unbounded): the kernels look for a neighbour within this many cutoffs (a query the
 * cutoff rejects keeps a seed and a temporal-cache bound; results are filtered by the cutoff afterwards, like the reference); "tie_rule" (0/1,
 * default 1): exact distance ties are decided the way nanoflann decides them (first visited target; 0 = lowest original index).  The rule is an INPUT of a
 * search: changing it drops the cross-round state and gives every edge a new epoch, like mvicp_reset_history.  The fix-up walks nanoflann's own tree
 * over the target, of any depth up to 16384 levels (a cloud whose coordinates form a geometric progression has one level per point; ordinary clouds
 * have 20-40); a deeper tree makes the call that needs it return MVICP_ERR_ARG — such a cloud can only be searched with "tie_rule" 0; "tie_lazy" (0/1, default 1;
 * single rank only, read at mvicp_set_graph): the reference-equivalent trees that decide ties are built when a search first reports a tie on a target
 * without one — that search is then repeated once — like the reference's own lazily built index (frame.cpp:188-193); 0 = built for every target at mvicp_set_graph; "sel_bracket" (0/1, default 1): one-pass median select around last round's median
 * once it has settled; "sel_reuse" (0/1, default 1; single rank): a search in which no list can change (every transform bit-identical to the last search's, every list
 * valid) launches no median select and reuses the last one's result (0: launch it in every search); "spec_eval" (0/1, default 1): mvicp_correspond queues the first linearization of the following
 * mvicp_optimize (same poses, previous solve's flags) behind its own kernels so the round waits once, not twice; "spec2_eval" (0/1, default 1; single rank): when a
 * search's poses are bit-identical to the last search's (a converged registration), the candidate evaluation of the last solve is queued as well — the fixed-point
 * round's solve then needs no further device launch and no second wait (used only if the solve asks for exactly those poses); "lin_pair" (0/1, default 1): those
 * two queued evaluations go as ONE paired launch that reads the operand stream once (see mvicp_linearize_pair; 0: two launches with a copy between them); "lin_share_p"
 * (0/1, default 1): the linearization reads the source points of an all-accepted edge from the shared sorted cloud; "lin_interleave" (0/1, default 1; read at
 * mvicp_set_graph): the linearization's workgroups of the edges that share a source cloud are launched interleaved in groups of 8, so that the second reader of a
 * piece of the cloud runs on the XCD whose L2 still holds it; "lin_tail_last" (0/1, default 1; read at mvicp_set_graph): every edge's full chunks are launched before
 * all partial last chunks, so that the workgroups that start last, and run almost alone, are the short ones; "nn_cell"
 * (0/1, default 0): wave-cooperative cell-staging variant of the grid kernel; "tile_bounds" (default 1): the MVICP_NN_AUTO round
 * that hands over from the tile kernel to the grid kernel runs a build of the tile kernel that also leaves the temporal-cache
 * bounds (2: every tile round does, 0: off), "tile_mu" (default 0.02): its guard band in hash-cell edges; "tile_cache" (0/1, default 1):
 * after that hand-over, rounds whose poses still move run the same build with the temporal-cache check as its prologue (lanes whose
 * neighbour provably did not change sit out; the wave searches for its missed lanes only) and the grid kernel only re-verifies the fixed point (2: the
 * prologue in EVERY tile round that follows a bounds-leaving one — an experiment, profiles/r06_tile_ab.txt); "reject_cache" (0/1, default 1): in those rounds a query whose old neighbour
 * AND every other target are provably beyond the cutoff after the pose update is a cache hit too (it stays rejected, frame.cpp:156; its exact neighbour is never
 * output) — the lanes with the largest search balls leave the traversal; "cache_mfma_ratio" (default 3; 0 = never): a cache-aware round runs on the
 * matrix-pipe build instead when the median displacement bound of the queries since the last search exceeds this many guard bands (low expected hit rate);
 * "tile_miss" (default 8; 0 = off): in those
 * cache-aware rounds a wave left with at most this many missed lanes answers them one by one with its 64 lanes spread over the tile boxes / the points
 * (nn_tile.hip miss_block); "mfma_entry" (0/1, default 0): seeded matrix-pipe launches enter at the blocks their seeds lie in and prove completeness with one
 * flat sweep over the block boxes instead of the top-down walk (an experiment: faster only once the poses have settled); "prune_rho", "auto_settle", "auto_switch",
 * see DESIGN.md; "grid_curve" (default 2): device order of the clouds at the next mvicp_set_frame, 2 = balanced k-d order,
 * 1 / 0 = Hilbert / Morton index of the hash cell (nn_cell needs 0 or 1).  Tuning knobs: correspondences are
 * bit-identical for every setting.
 * ONLY ON 3-LEVEL TARGETS: "mfma_entry", "tile_waves" 7 (nn_tile_kernel) / 4 / 6 (nn_mfma_kernel) and "mfma_lbt" (1: the per-lane box test of unseeded
 * launches, >= 2: also in cache-aware matrix-pipe rounds) select builds that exist only for a launch whose targets all have three box levels (131 073 ..
 * 8 388 608 points each); at any other depth they are accepted and the launch runs the 2-level or the generic build of the same search ("tile_waves" 8 has a
 * generic build as well).  mvicp_last_nn_launch says which build ran.
 * Non-OK returns: a NULL or unknown name, a value outside the range its option states ("match_chunk" outside [1, 2^31), "grid_target"
 * outside [0.5, 64], "tile_mu" outside (0, 1], "mfma_kacc" outside [1, 1024], "tile_miss" outside [0, 64], "nn_search_factor" < 0) ->
 * MVICP_ERR_ARG; the option keeps its value. */
int mvicp_set_option(mvicp_ctx* ctx, const char* name, double value);
/* NN census accumulated while profiling and the "nn_census" option are on: counters in this order — queries, candidate points
 * examined, tree boxes / grid cells looked up, queries that needed the tree fallback, queries answered by the temporal cache,
 * candidate points fetched from memory (a wave-cooperative kernel fetches a point once and examines it from LDS many times). */
int mvicp_nn_census(mvicp_ctx* ctx, double* out5);              /* the first five counters (the 0.1 contract) */
/* All counters the build has, at most `cap` of them; returns how many were written (10 since version 0.4) or a negative status. */
int mvicp_nn_census_ex(mvicp_ctx* ctx, double* out, int cap);
/* Which NN kernel the last search of this context launched (mvicp_correspond, mvicp_nn_query; "" before the first, or for a NULL context):
 * "brute", "grid", "tile<WPE,TOP,BND>" (nn_tile_kernel) or "mfma<WPE,TOP,BND,CEN,LBT,ENTRY>" (nn_mfma_kernel) with the template arguments of
 * the instantiation as integers — WPE waves per SIMD, TOP + 1 box levels (-1: the generic build), then 0/1 flags: BND leaves temporal-cache
 * bounds, CEN counts the census, LBT per-lane box test per tile, ENTRY enters at the seeds' blocks.  The string lives in the context and is
 * overwritten by the next search.  Host state only: no device call, never fails. */
const char* mvicp_last_nn_launch(mvicp_ctx* ctx);

/* ---- profiling (HIP events on the library's own stream) ------------------------------------------ */
/* on = 0: off; 1: every scope below; 2: only the NN kernels, "linearize", "linearize_pair" and "comm" (fewer event packets between the kernels of
 * a timed run). */
int mvicp_profile_enable(mvicp_ctx* ctx, int on);
int mvicp_profile_reset(mvicp_ctx* ctx);
/* kernel in {"nn_brute","nn_grid","nn_tile","nn_mfma" (one scope per NN kernel; "nn" = all of them together),"compact","gather","select","linearize",
 * "reduce","comm"} (HIP-event scopes) or a host timer ("host.correspond", "host.optimize", "host.evaluate", ...) or "spec.hit" (first evaluations
 * served by the queued launch: launches only): total ms, launches, bytes of the library's own model. */
int mvicp_profile_get(mvicp_ctx* ctx, const char* kernel, double* total_ms, long long* launches, double* alg_bytes);
/* The same entry as numbers: out[0..4] = total ms, launches, model bytes, SURVEY 8(d) algorithmic bytes (NN scopes: 36 B per query + 24 B per
 * candidate point fetched + 8 B per box or cell looked up; the last two need the "nn_census" option), queries answered.  Returns how many were written. */
int mvicp_profile_get_ex(mvicp_ctx* ctx, const char* kernel, double* out, int cap);
/* Opaque hipStream_t the library launches on (so a harness can bracket it with its own events). */
void* mvicp_stream(mvicp_ctx* ctx);
int mvicp_sync(mvicp_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MVICP_H */
