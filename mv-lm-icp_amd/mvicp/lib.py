"""ctypes binding of include/mvicp.h.  No compute happens here; every call goes through the C ABI."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MVICP_LIB") or os.path.join(os.path.dirname(_HERE), "libmvicp_hip.so")   # MVICP_LIB: tuning builds only

PARAM_EIGEN_QUATERNION, PARAM_ANGLE_AXIS, PARAM_SOPHUS_SE3 = 0, 1, 2
METRIC_POINT, METRIC_PLANE, METRIC_SYMMETRIC = 0, 1, 2   # mvicp_metric
NN_AUTO, NN_BRUTE, NN_GRID, NN_TILE = 0, 1, 2, 3
ORIENT_ANCHOR, ORIENT_VIEWPOINT, ORIENT_DIRECTION = 0, 1, 2   # mvicp_orient_mode
REJECT_AS_TARGET, REJECT_AS_SOURCE = 1, 2   # roles of a reject mask (mvicp_set_reject_mask), may be or-ed
EDGE_BLOCK = 91

SYMBOLS = [
    "mvicp_last_error", "mvicp_version", "mvicp_create", "mvicp_destroy", "mvicp_set_num_frames", "mvicp_set_frame",
    "mvicp_recompute_normals", "mvicp_set_graph", "mvicp_set_shard", "mvicp_edge_owner", "mvicp_comm_unique_id", "mvicp_comm_init", "mvicp_comm_nranks", "mvicp_comm_set_callback", "mvicp_correspond",
    "mvicp_get_correspondences", "mvicp_map_correspondences", "mvicp_map_correspondences_async", "mvicp_wait_correspondences", "mvicp_correspondence_epochs", "mvicp_set_correspondences", "mvicp_nn_query", "mvicp_linearize", "mvicp_linearize_pair", "mvicp_linearize_metric", "mvicp_linearize_gicp", "mvicp_optimize", "mvicp_optimize_metric", "mvicp_optimize_gicp",
    "mvicp_lm_solve", "mvicp_set_option", "mvicp_nn_census", "mvicp_nn_census_ex", "mvicp_last_nn_launch", "mvicp_reset_history", "mvicp_profile_enable", "mvicp_profile_reset", "mvicp_profile_get", "mvicp_profile_get_ex", "mvicp_stream", "mvicp_sync",
    "mvicp_closedform_point_to_point", "mvicp_closedform_point_to_plane", "mvicp_set_frame_device", "mvicp_get_structure",
    "mvicp_overlap", "mvicp_graph_from_overlap", "mvicp_voxel_grid", "mvicp_voxel_fetch",
    "mvicp_outlier_filter", "mvicp_outlier_fetch", "mvicp_outlier_threshold", "mvicp_cache_allowance",
    "mvicp_cluster", "mvicp_cluster_fetch", "mvicp_cluster_keep_rule", "mvicp_cluster_select", "mvicp_cluster_fetch_kept",
    "mvicp_segment_plane", "mvicp_plane_fetch", "mvicp_plane_select", "mvicp_plane_fetch_kept", "mvicp_plane_from_moments",
    "mvicp_boundary", "mvicp_boundary_fetch", "mvicp_boundary_select", "mvicp_boundary_fetch_kept",
    "mvicp_set_reject_mask", "mvicp_boundary_adopt", "mvicp_get_reject_mask",
    "mvicp_knn_search", "mvicp_knn_fetch", "mvicp_fpfh", "mvicp_fpfh_fetch", "mvicp_iss_keypoints", "mvicp_iss_fetch",
    "mvicp_estimate_normals", "mvicp_normals_fetch", "mvicp_normals_adopt", "mvicp_fit_normals", "mvicp_normals_fit_fetch",
    "mvicp_smooth_points", "mvicp_smooth_fetch",
    "mvicp_orient_normals", "mvicp_orient_fetch", "mvicp_orient_adopt", "mvicp_normal_agreement", "mvicp_signs_from_agreement", "mvicp_negate_normals",
    "mvicp_feature_match", "mvicp_feature_match_fetch", "mvicp_match_pairs", "mvicp_consensus", "mvicp_consensus_fetch",
    "mvicp_coarse_pairs", "mvicp_coarse_pairs_fetch", "mvicp_poses_from_pairs",
]

# names of mvicp_get_structure (include/mvicp.h)
STRUCTURE_NAMES = ("spts", "sidx", "srec", "crec", "inv", "snor", "table", "oct", "wide", "mf_ops", "mf_blk", "bricks", "celltab",
                   "h_order", "h_inv", "scalars")


class MvicpError(RuntimeError):
    pass


class Summary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("termination", C.c_int), ("evaluations", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OutlierStats(C.Structure):
    _fields_ = [("n", C.c_longlong), ("kept", C.c_longlong), ("q_exp", C.c_int), ("has_normals", C.c_int), ("s1", C.c_ulonglong),
                ("s2_hi", C.c_ulonglong), ("s2_lo", C.c_ulonglong), ("T", C.c_double), ("threshold", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["s2"] = (d["s2_hi"] << 64) | d["s2_lo"]
        return d


class ClusterStats(C.Structure):
    _fields_ = [("n", C.c_longlong), ("clusters", C.c_longlong), ("core", C.c_longlong), ("border", C.c_longlong), ("noise", C.c_longlong),
                ("largest", C.c_longlong), ("largest_label", C.c_int), ("has_normals", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PlaneResult(C.Structure):
    _fields_ = [("best", C.c_int), ("count", C.c_int), ("accepted", C.c_int), ("refit", C.c_int), ("count_refined", C.c_int), ("b", C.c_int),
                ("q", C.c_int), ("has_normals", C.c_int), ("n", C.c_longlong), ("normal", C.c_double * 3), ("point", C.c_double * 3),
                ("d", C.c_double), ("hyp_normal", C.c_double * 3), ("hyp_point", C.c_double * 3)]

    def as_dict(self):
        vec = ("normal", "point", "hyp_normal", "hyp_point")
        return {k: np.array(getattr(self, k)) if k in vec else getattr(self, k) for k, _ in self._fields_}


class ConsensusResult(C.Structure):
    _fields_ = [("best", C.c_int), ("count", C.c_int), ("accepted", C.c_int), ("reserved", C.c_int), ("pose", C.c_double * 16)]


class CoarseEdge(C.Structure):
    _fields_ = [("pairs", C.c_int), ("best", C.c_int), ("count", C.c_int), ("accepted", C.c_int), ("pose", C.c_double * 16)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t)
EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))

_lib = None


def load_library(path=None):
    """Load libmvicp_hip.so (fails loudly if it has not been built: there is no Python/CPU fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise MvicpError(f"{p} not found: build it with `make -C mv-lm-icp_amd` (or __graft_entry__.build())")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    vp, ip, dp, fp, u8p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    lib.mvicp_last_error.restype = C.c_char_p
    lib.mvicp_version.restype = C.c_char_p
    lib.mvicp_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.mvicp_destroy.argtypes = [vp]
    lib.mvicp_set_num_frames.argtypes = [vp, C.c_int]
    lib.mvicp_set_frame.argtypes = [vp, C.c_int, dp, dp, C.c_int]
    lib.mvicp_recompute_normals.argtypes = [vp, C.c_int, C.c_int, dp, ip]
    lib.mvicp_set_graph.argtypes = [vp, C.c_int, ip, ip]
    lib.mvicp_set_shard.argtypes = [vp, C.c_int, C.c_int]
    lib.mvicp_edge_owner.argtypes = [C.c_int, ip, C.c_int, ip]
    lib.mvicp_comm_unique_id.argtypes = [C.c_char_p, vp]
    lib.mvicp_comm_init.argtypes = [vp, C.c_char_p, vp, C.c_int, C.c_int]
    lib.mvicp_comm_set_callback.argtypes = [vp, ALLREDUCE_FN, vp]
    lib.mvicp_comm_nranks.argtypes = [vp]
    lib.mvicp_correspond.argtypes = [vp, dp, u8p, C.c_float, C.c_int, ip, fp]
    lib.mvicp_get_correspondences.argtypes = [vp, C.c_int, C.c_int, ip, ip, dp]
    lib.mvicp_map_correspondences.argtypes = [vp, C.POINTER(vp), C.POINTER(C.POINTER(C.c_longlong))]
    lib.mvicp_map_correspondences_async.argtypes = [vp, C.POINTER(vp), C.POINTER(C.POINTER(C.c_longlong))]
    lib.mvicp_wait_correspondences.argtypes = [vp, C.c_int]
    lib.mvicp_correspondence_epochs.argtypes = [vp, C.POINTER(C.POINTER(C.c_ulonglong))]
    lib.mvicp_set_correspondences.argtypes = [vp, C.c_int, C.c_int, ip, ip, C.c_float]
    lib.mvicp_nn_query.argtypes = [vp, C.c_int, dp, C.c_int, C.c_int, ip, dp]
    lib.mvicp_linearize.argtypes = [vp, dp, C.c_int, C.c_int, dp]
    lib.mvicp_linearize_pair.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp, dp]
    lib.mvicp_optimize.argtypes = [vp, dp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Summary)]
    lib.mvicp_linearize_metric.argtypes = [vp, dp, C.c_int, C.c_int, dp]
    lib.mvicp_optimize_metric.argtypes = [vp, dp, u8p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Summary)]
    lib.mvicp_linearize_gicp.argtypes = [vp, dp, C.c_double, C.c_int, dp]
    lib.mvicp_optimize_gicp.argtypes = [vp, dp, u8p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(Summary)]
    lib.mvicp_lm_solve.argtypes = [C.c_int, C.c_int, ip, ip, dp, u8p, C.c_int, C.c_int, EVAL_FN, vp, C.POINTER(Summary)]
    lib.mvicp_set_option.argtypes = [vp, C.c_char_p, C.c_double]
    lib.mvicp_nn_census.argtypes = [vp, dp]
    lib.mvicp_nn_census_ex.argtypes = [vp, dp, C.c_int]
    lib.mvicp_last_nn_launch.argtypes = [vp]
    lib.mvicp_last_nn_launch.restype = C.c_char_p
    lib.mvicp_reset_history.argtypes = [vp]
    lib.mvicp_profile_enable.argtypes = [vp, C.c_int]
    lib.mvicp_profile_reset.argtypes = [vp]
    lib.mvicp_profile_get.argtypes = [vp, C.c_char_p, dp, C.POINTER(C.c_longlong), dp]
    lib.mvicp_profile_get_ex.argtypes = [vp, C.c_char_p, dp, C.c_int]
    lib.mvicp_stream.argtypes = [vp]
    lib.mvicp_stream.restype = vp
    lib.mvicp_sync.argtypes = [vp]
    lib.mvicp_closedform_point_to_point.argtypes = [dp, dp, C.c_int, dp]
    lib.mvicp_closedform_point_to_plane.argtypes = [dp, dp, dp, C.c_int, dp]
    lib.mvicp_set_frame_device.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.mvicp_get_structure.argtypes = [vp, C.c_int, C.c_char_p, vp, C.c_longlong]
    lib.mvicp_get_structure.restype = C.c_longlong
    llp = C.POINTER(C.c_longlong)
    lib.mvicp_overlap.argtypes = [vp, dp, C.c_float, C.c_int, ip, ip, llp, ip]
    lib.mvicp_graph_from_overlap.argtypes = [C.c_int, ip, ip, llp, C.c_int, C.c_double, C.c_int, C.c_int, ip, ip, ip]
    lib.mvicp_voxel_grid.argtypes = [vp, C.c_int, ip, dp, C.c_double, ip]
    lib.mvicp_voxel_grid.restype = C.c_longlong
    lib.mvicp_voxel_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp]
    lib.mvicp_outlier_filter.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(OutlierStats)]
    lib.mvicp_outlier_filter.restype = C.c_longlong
    lib.mvicp_outlier_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp, C.c_longlong, vp, vp]
    lib.mvicp_outlier_threshold.argtypes = [C.c_longlong, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_double, dp]
    lib.mvicp_cluster.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.POINTER(ClusterStats)]
    lib.mvicp_cluster.restype = C.c_longlong
    lib.mvicp_cluster_fetch.argtypes = [vp, C.c_longlong, vp, vp, C.c_longlong, vp]
    lib.mvicp_cluster_keep_rule.argtypes = [C.c_longlong, vp, C.c_longlong, C.c_longlong, vp]
    lib.mvicp_cluster_select.argtypes = [vp, C.c_longlong, C.c_longlong]
    lib.mvicp_cluster_select.restype = C.c_longlong
    lib.mvicp_cluster_fetch_kept.argtypes = [vp, C.c_longlong, vp, vp, vp, vp]
    lib.mvicp_segment_plane.argtypes = [vp, C.c_int, C.c_longlong, C.c_ulonglong, C.c_double, dp, C.c_double, C.c_int, C.POINTER(PlaneResult)]
    lib.mvicp_plane_fetch.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp]
    lib.mvicp_plane_select.argtypes = [vp, C.c_int]
    lib.mvicp_plane_select.restype = C.c_longlong
    lib.mvicp_plane_fetch_kept.argtypes = [vp, C.c_longlong, vp, vp, vp]
    lib.mvicp_plane_from_moments.argtypes = [C.c_longlong, vp, vp, C.c_int, dp, dp, dp, dp]
    lib.mvicp_boundary.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.mvicp_boundary.restype = C.c_longlong
    lib.mvicp_boundary_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp, vp]
    lib.mvicp_boundary_select.argtypes = [vp, C.c_int]
    lib.mvicp_boundary_select.restype = C.c_longlong
    lib.mvicp_boundary_fetch_kept.argtypes = [vp, C.c_longlong, vp, vp, vp]
    lib.mvicp_set_reject_mask.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.mvicp_boundary_adopt.argtypes = [vp, C.c_int]
    lib.mvicp_get_reject_mask.argtypes = [vp, C.c_int, vp, C.c_longlong, ip]
    lib.mvicp_get_reject_mask.restype = C.c_longlong
    lib.mvicp_cache_allowance.argtypes =[dp, dp, dp, dp, C.c_double, dp]
    lib.mvicp_knn_search.argtypes = [vp, C.c_int, vp, C.c_longlong, C.c_int, C.c_double]
    lib.mvicp_knn_search.restype = C.c_longlong
    lib.mvicp_knn_fetch.argtypes = [vp, C.c_longlong, C.c_longlong, vp, vp, vp, vp]
    lib.mvicp_fpfh.argtypes = [vp, C.c_int, C.c_double, C.c_int]
    lib.mvicp_fpfh.restype = C.c_longlong
    lib.mvicp_fpfh_fetch.argtypes = [vp, C.c_longlong, vp, vp]
    lib.mvicp_iss_keypoints.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]
    lib.mvicp_iss_keypoints.restype = C.c_longlong
    lib.mvicp_iss_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp, C.c_longlong, vp, vp, vp]
    lib.mvicp_estimate_normals.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp]
    lib.mvicp_estimate_normals.restype = C.c_longlong
    lib.mvicp_normals_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp]
    lib.mvicp_normals_adopt.argtypes = [vp]
    lib.mvicp_fit_normals.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp, C.c_int]
    lib.mvicp_fit_normals.restype = C.c_longlong
    lib.mvicp_normals_fit_fetch.argtypes = [vp, C.c_longlong, vp]
    lib.mvicp_smooth_points.argtypes = [vp, C.c_int, C.c_int, C.c_double, dp, C.c_int, C.c_double]
    lib.mvicp_smooth_points.restype = C.c_longlong
    lib.mvicp_smooth_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp, vp, vp]
    lib.mvicp_orient_normals.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp]
    lib.mvicp_orient_normals.restype = C.c_longlong
    lib.mvicp_orient_fetch.argtypes = [vp, C.c_longlong, vp, vp, vp]
    lib.mvicp_orient_adopt.argtypes = [vp]
    lib.mvicp_normal_agreement.argtypes = [vp, dp, ip, ip]
    lib.mvicp_signs_from_agreement.argtypes = [C.c_int, C.c_int, ip, ip, ip, ip, C.c_int, C.POINTER(C.c_ubyte), ip]
    lib.mvicp_negate_normals.argtypes = [vp, C.c_int]
    lib.mvicp_feature_match.argtypes = [vp, vp, C.c_longlong, vp, C.c_longlong, C.c_int]
    lib.mvicp_feature_match.restype = C.c_longlong
    lib.mvicp_feature_match_fetch.argtypes = [vp, C.c_longlong, C.c_longlong, vp, vp, vp, vp]
    lib.mvicp_match_pairs.argtypes = [C.c_longlong, C.c_longlong, vp, vp, vp, C.c_int, C.c_double, vp]
    lib.mvicp_match_pairs.restype = C.c_longlong
    lib.mvicp_consensus.argtypes = [vp, vp, vp, C.c_longlong, C.c_longlong, C.c_ulonglong, C.c_double, C.c_double, C.POINTER(ConsensusResult)]
    lib.mvicp_consensus_fetch.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp]
    lib.mvicp_coarse_pairs.argtypes = [vp, vp, vp, llp, C.c_int, C.c_int, C.c_int, ip, ip, C.POINTER(C.c_ulonglong), C.c_int, C.c_double,
                                       C.c_longlong, C.c_double, C.c_double, C.POINTER(CoarseEdge)]
    lib.mvicp_coarse_pairs.restype = C.c_longlong
    lib.mvicp_coarse_pairs_fetch.argtypes = [vp, C.c_int, C.c_longlong, vp, vp]
    lib.mvicp_poses_from_pairs.argtypes = [C.c_int, C.c_int, ip, ip, ip, dp, C.c_int, C.c_int, dp, dp, ip, ip, ip]
    if path is None:
        _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def check_device_cloud(t, device, n=None, name="xyz"):
    """The checks of a device cloud for Engine.set_frame_device, before any library call: a torch tensor, float64, shape (n, 3),
    contiguous, on the GPU `device` (an index).  Raises TypeError / ValueError; returns the number of points."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be float64, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must have shape (n, 3), got {tuple(t.shape)}")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} has {t.shape[0]} rows, the cloud {n}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not t.is_cuda:
        raise TypeError(f"{name} must be a GPU (HIP) tensor, got device {t.device}")
    if t.device.index != device:
        raise ValueError(f"{name} is on cuda:{t.device.index}, the engine on cuda:{device}")
    return int(t.shape[0])


def _check(lib, st):
    if st < 0:
        raise MvicpError(f"mvicp status {st}: {lib.mvicp_last_error().decode()}")
    return st


def poses_to_c(poses):
    """(K,4,4) row-major numpy matrices -> K x 16 column-major doubles (Eigen Isometry3d::data())."""
    P = np.asarray(poses, dtype=np.float64)
    return np.ascontiguousarray(np.transpose(P, (0, 2, 1)).reshape(len(P), 16))


def poses_from_c(buf):
    return np.ascontiguousarray(np.transpose(np.asarray(buf, dtype=np.float64).reshape(-1, 4, 4), (0, 2, 1)))


def edge_owner(n_src, world):
    lib = load_library()
    n_src = np.ascontiguousarray(n_src, dtype=np.int32)
    owner = np.zeros(len(n_src), dtype=np.int32)
    _check(lib, lib.mvicp_edge_owner(len(n_src), _ip(n_src), world, _ip(owner)))
    return owner


def overlap_sample_indices(n, max_samples):
    """The sample rule of mvicp_overlap: ORIGINAL indices of the s sample points of a cloud of n points, s = n if max_samples <= 0 or
    max_samples >= n else max_samples; the t-th is floor(t * n / s) in 64-bit integers."""
    n = int(n)
    s = n if max_samples <= 0 or max_samples >= n else int(max_samples)
    if s == 0:
        return np.zeros(0, dtype=np.int64)
    return (np.arange(s, dtype=np.int64) * n) // s


def graph_from_overlap(samples, hits, sumq=None, knn=2, min_fraction=0.0, skip_fixed0=True, cap=None):
    """mvicp_graph_from_overlap: frame i keeps the knn frames with the most hits (ties: smaller sumq, then lower index) among those with
    hits > 0 and hits >= min_fraction * samples[i].  -> (src, dst, n_components); edges src ascending, neighbours best first;
    skip_fixed0 omits the edges out of frame 0.  cap (default K * min(knn, K - 1)): capacity of the edge arrays; more edges raise."""
    lib = load_library()
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    K = len(samples)
    hits = np.ascontiguousarray(hits, dtype=np.int32).reshape(K, K)
    sq = None if sumq is None else np.ascontiguousarray(sumq, dtype=np.int64).reshape(K, K)
    if cap is None:
        cap = K * max(min(int(knn), K - 1), 0)
    src = np.zeros(max(cap, 1), dtype=np.int32); dst = np.zeros(max(cap, 1), dtype=np.int32)
    nc = C.c_int(0)
    n = _check(lib, lib.mvicp_graph_from_overlap(K, _ip(samples), _ip(hits), sq.ctypes.data_as(C.POINTER(C.c_longlong)) if sq is not None else None,
                                                 int(knn), float(min_fraction), int(bool(skip_fixed0)), int(cap), _ip(src), _ip(dst), C.byref(nc)))
    return src[:n].copy(), dst[:n].copy(), int(nc.value)


def outlier_threshold(n, s1, s2, std_ratio):
    """mvicp_outlier_threshold: the threshold T (quantised units) of the statistical outlier rule from the exact integer sums
    S1 = sum M_i and S2 = sum M_i^2 (Python integers; S2 up to 128 bits) over n points.  Host only."""
    lib = load_library()
    s1, s2 = int(s1), int(s2)
    if not (0 <= s1 < 1 << 64 and 0 <= s2 < 1 << 128):
        raise ValueError("s1 must fit 64 bits and s2 128 bits")
    T = C.c_double(0.0)
    _check(lib, lib.mvicp_outlier_threshold(int(n), s1, s2 >> 64, s2 & ((1 << 64) - 1), float(std_ratio), C.byref(T)))
    return T.value


def cluster_keep_rule(size, min_size=0, max_clusters=0):
    """mvicp_cluster_keep_rule: which clusters stay, from their sizes (index = label).  The clusters are ranked by (size descending, label
    ascending); keep[c] = size[c] >= min_size and (max_clusters == 0 or rank(c) < max_clusters) -> (C,) uint8.  Host only."""
    lib = load_library()
    size = np.ascontiguousarray(size, dtype=np.int32).reshape(-1)
    n = len(size)
    src = np.concatenate([size, np.zeros(1, dtype=np.int32)])   # (never a NULL pointer for C = 0)
    keep = np.zeros(n + 1, dtype=np.uint8)
    _check(lib, lib.mvicp_cluster_keep_rule(n, src.ctypes.data_as(C.c_void_p), int(min_size), int(max_clusters), keep.ctypes.data_as(C.c_void_p)))
    return keep[:n].copy()


def plane_from_moments(c, s, S, q, a, m):
    """mvicp_plane_from_moments: the refit rule of mvicp_segment_plane from the exact integer sums on -- c inliers, s (3) = sum M_k,
    S (6) = sum M_k M_l in the order 00 01 02 11 12 22, q the scale exponent, a / m the hypothesis's point and unit normal
    -> (normal (3,), point (3,)).  Host only."""
    lib = load_library()
    s = np.ascontiguousarray(s, dtype=np.int64).reshape(3)
    S = np.ascontiguousarray(S, dtype=np.int64).reshape(6)
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(3)
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(3)
    normal, point = np.zeros(3), np.zeros(3)
    _check(lib, lib.mvicp_plane_from_moments(int(c), s.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p), int(q), _dp(a), _dp(m), _dp(normal), _dp(point)))
    return normal, point


def reject_by_mask(first, second, src_mask, dst_mask):
    """The pairs (first[i], second[i]) neither of whose ends is flagged, in their order: src_mask / dst_mask are per-point flags of the
    source / target cloud (nonzero = reject every pair on that point; the flag of Engine.boundary, say), either may be None.
    -> (first, second) int32.  Pure numpy; the filter of Engine.reject_correspondences."""
    first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    second = np.ascontiguousarray(second, dtype=np.int32).reshape(-1)
    if len(first) != len(second):
        raise ValueError("first and second differ in length")
    keep = np.ones(len(first), dtype=bool)
    if src_mask is not None:
        keep &= np.asarray(src_mask).reshape(-1)[first] == 0
    if dst_mask is not None:
        keep &= np.asarray(dst_mask).reshape(-1)[second] == 0
    return np.ascontiguousarray(first[keep]), np.ascontiguousarray(second[keep])


def cache_allowance(pose_src_old, pose_dst_old, pose_src, pose_dst, max_norm):
    """mvicp_cache_allowance: the rounding allowance the temporal cache adds to an edge's query displacement between the search at
    the old pose pair and the one at the new pair (4x4 matrices), for a source cloud with max |p| <= max_norm.  Host only."""
    lib = load_library()
    P = poses_to_c(np.stack([np.asarray(a, dtype=np.float64).reshape(4, 4) for a in (pose_src_old, pose_dst_old, pose_src, pose_dst)]))
    out = C.c_double(0.0)
    _check(lib, lib.mvicp_cache_allowance(_dp(P[0]), _dp(P[1]), _dp(P[2]), _dp(P[3]), float(max_norm), C.byref(out)))
    return out.value


def closedform_point_to_point(src, dst):
    """ICP_Closedform::pointToPoint (icp-closedform.cpp:9-26): least-squares rigid transform src -> dst.  Host only."""
    lib = load_library()
    a = np.ascontiguousarray(src, dtype=np.float64); b = np.ascontiguousarray(dst, dtype=np.float64)
    out = np.zeros(16)
    _check(lib, lib.mvicp_closedform_point_to_point(_dp(a), _dp(b), len(a), _dp(out)))
    return poses_from_c(out)[0]


def closedform_point_to_plane(src, dst, nor):
    """ICP_Closedform::pointToPlane (icp-closedform.cpp:30-54): one linearised point-to-plane step from identity.  Host only."""
    lib = load_library()
    a = np.ascontiguousarray(src, dtype=np.float64); b = np.ascontiguousarray(dst, dtype=np.float64); c = np.ascontiguousarray(nor, dtype=np.float64)
    out = np.zeros(16)
    _check(lib, lib.mvicp_closedform_point_to_plane(_dp(a), _dp(b), _dp(c), len(a), _dp(out)))
    return poses_from_c(out)[0]


def match_pairs(fwd_idx, fwd_d2, bwd_idx, mutual=True, ratio=1.0):
    """mvicp_match_pairs on the fetched arrays of Engine.feature_match: pair (i, j = fwd_idx[i][0]) is kept iff j >= 0, (not mutual or
    bwd_idx[j][0] == i) and (ratio >= 1 or fwd_d2[i][0] <= ratio^2 fwd_d2[i][1]) -> (k, 2) int32, ascending i.  Host only."""
    lib = load_library()
    fi = np.ascontiguousarray(fwd_idx, dtype=np.int32).reshape(-1, 2)
    fd = np.ascontiguousarray(fwd_d2, dtype=np.float64).reshape(-1, 2)
    bi = np.ascontiguousarray(bwd_idx, dtype=np.int32).reshape(-1, 2)
    if len(fd) != len(fi):
        raise ValueError("fwd_idx and fwd_d2 differ in length")
    m, n = len(fi), len(bi)
    pairs = np.zeros((max(m, 1), 2), dtype=np.int32)
    spare = np.zeros(2)   # (an empty array still gets a pointer that is not NULL)
    ptr = lambda a: (a if a.size else spare).ctypes.data_as(C.c_void_p)
    k = _check(lib, lib.mvicp_match_pairs(m, n, ptr(fi), ptr(fd), ptr(bi), int(bool(mutual)), float(ratio), ptr(pairs)))
    return pairs[:k].copy()


def coarse_align(eng, src_frame, dst_frame, src_xyz, dst_xyz, radius, max_nn=64, hypotheses=10000, seed=0, tau=None, edge_sim=0.9,
                 mutual=True, ratio=1.0):
    """A coarse pose src -> dst from the clouds alone: Engine.fpfh of both frames (device results) -> Engine.feature_match ->
    match_pairs -> Engine.consensus -> closedform_point_to_point over the winner's inliers in ascending pair order (when there are at
    least 3).  src_xyz / dst_xyz: the stored clouds of the two frames as numpy arrays; tau: the inlier distance of the consensus.
    -> dict(pose (4,4) = the consensus pose, refined (4,4), pairs (k,2), inliers (k,) uint8, counts = dict(pairs, accepted, inliers,
    best)).  Fewer than 3 pairs, or no accepted hypothesis: both poses are the identity and best = -1."""
    if tau is None:
        raise ValueError("coarse_align needs tau, the inlier distance of the consensus")
    src_xyz = np.ascontiguousarray(src_xyz, dtype=np.float64).reshape(-1, 3)
    dst_xyz = np.ascontiguousarray(dst_xyz, dtype=np.float64).reshape(-1, 3)
    da = eng.fpfh(src_frame, radius, max_nn, device=True)["desc"]
    db = eng.fpfh(dst_frame, radius, max_nn, device=True)["desc"]
    if da.shape[0] != len(src_xyz) or db.shape[0] != len(dst_xyz):
        raise ValueError("src_xyz / dst_xyz are not the clouds of the two frames")
    mt = eng.feature_match(da, db)
    pairs = match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, ratio)
    out = {"pose": np.eye(4), "refined": np.eye(4), "pairs": pairs, "inliers": np.zeros(len(pairs), dtype=np.uint8),
           "counts": {"pairs": len(pairs), "accepted": 0, "inliers": 0, "best": -1}}
    if len(pairs) < 3:
        return out
    P, Q = np.ascontiguousarray(src_xyz[pairs[:, 0]]), np.ascontiguousarray(dst_xyz[pairs[:, 1]])
    cons = eng.consensus(P, Q, hypotheses, seed, tau, edge_sim)
    out["pose"], out["inliers"] = cons["pose"], cons["flags"]
    out["counts"].update(accepted=cons["accepted"], inliers=cons["count"], best=cons["best"])
    keep = cons["flags"] != 0
    out["refined"] = closedform_point_to_point(P[keep], Q[keep]) if cons["count"] >= 3 else cons["pose"].copy()
    return out


def poses_from_pairs(n_frames, src, dst, count, pose, min_count=0, root=0, root_pose=None):
    """mvicp_poses_from_pairs: initial poses (frame -> world) from pairwise poses.  pose[e] (4, 4) maps coordinates of frame src[e] into
    those of dst[e]; edge e is usable iff count[e] >= min_count.  A maximum spanning forest from `root` (Prim: the largest count, the
    lowest e among equals); a frame no usable edge reaches starts a component of its own at the identity.
    -> dict(poses (K,4,4), parent (K,), parent_edge (K,), component (K,), components).  Host only."""
    lib = load_library()
    src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1); dst = np.ascontiguousarray(dst, dtype=np.int32).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.int32).reshape(-1)
    E = len(src)
    if len(dst) != E or len(count) != E:
        raise ValueError("src, dst and count differ in length")
    T = poses_to_c(np.asarray(pose, dtype=np.float64).reshape(E, 4, 4)) if E else np.zeros((1, 16))
    K = int(n_frames)
    out = np.zeros((max(K, 1), 16)); parent = np.zeros(max(K, 1), dtype=np.int32); pedge = np.zeros(max(K, 1), dtype=np.int32)
    comp = np.zeros(max(K, 1), dtype=np.int32)
    rp = None if root_pose is None else poses_to_c(np.asarray(root_pose, dtype=np.float64).reshape(1, 4, 4))
    spare = np.zeros(1, dtype=np.int32)   # (an empty array still gets a pointer that is not NULL)
    ip = lambda a: _ip(a if a.size else spare)
    nc = _check(lib, lib.mvicp_poses_from_pairs(K, E, ip(src), ip(dst), ip(count), _dp(T), int(min_count), int(root), None if rp is None else _dp(rp),
                                                _dp(out), _ip(parent), _ip(pedge), _ip(comp)))
    return {"poses": poses_from_c(out[:K]), "parent": parent[:K].copy(), "parent_edge": pedge[:K].copy(), "component": comp[:K].copy(),
            "components": int(nc)}


def principal_curvatures(H, K):
    """The principal curvatures (k1 >= k2) from the mean curvature H and the Gaussian curvature K of Engine.smooth_points: D = H * H - K (a
    negative D, which only rounding produces, counts as 0), r = sqrt(D) -> (H + r, H - r).  numpy only."""
    H, K = np.asarray(H, dtype=np.float64), np.asarray(K, dtype=np.float64)
    D = H * H - K
    r = np.sqrt(np.where(D < 0, 0.0, D))
    return H + r, H - r


def signs_from_agreement(n_frames, src, dst, pos, neg, min_count=0):
    """mvicp_signs_from_agreement: which frames to negate so that the normals of all frames agree.  Edge e = (src[e], dst[e]) with pos[e]
    pairs whose normals agree and neg[e] that disagree is usable iff pos + neg >= min_count and pos != neg; the maximum spanning forest by
    (|pos - neg| descending, e ascending); every tree's lowest frame keeps its sign.
    -> dict(flip (K,) uint8, component (K,) int32 = the lowest frame of the tree, components).  Host only."""
    lib = load_library()
    src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1); dst = np.ascontiguousarray(dst, dtype=np.int32).reshape(-1)
    pos = np.ascontiguousarray(pos, dtype=np.int32).reshape(-1); neg = np.ascontiguousarray(neg, dtype=np.int32).reshape(-1)
    E = len(src)
    if len(dst) != E or len(pos) != E or len(neg) != E:
        raise ValueError("src, dst, pos and neg differ in length")
    K = int(n_frames)
    flip = np.zeros(max(K, 1), dtype=np.uint8); comp = np.zeros(max(K, 1), dtype=np.int32)
    spare = np.zeros(1, dtype=np.int32)   # (an empty array still gets a pointer that is not NULL)
    ip = lambda a: _ip(a if a.size else spare)
    nc = _check(lib, lib.mvicp_signs_from_agreement(K, E, ip(src), ip(dst), ip(pos), ip(neg), int(min_count), flip.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                    _ip(comp)))
    return {"flip": flip[:K].copy(), "component": comp[:K].copy(), "components": int(nc)}


def orient_frames(eng, poses, fixed, cutoff, min_count=0):
    """The cross-frame step of a consistent orientation, on an engine with a graph whose frames all have normals (each consistent in
    itself: Engine.orient_normals + adopt_orientation): correspond(poses, fixed, cutoff) -> normal_agreement(poses) ->
    signs_from_agreement over the engine's edges -> negate_normals on every frame the rule flips -> reset_history, so that the
    registration that follows is an ordinary one.  -> dict(flip, component, components, pos, neg, counts)."""
    counts, _ = eng.correspond(poses, fixed, cutoff)
    pos, neg = eng.normal_agreement(poses)
    out = signs_from_agreement(len(eng.npts), eng.src, eng.dst, pos, neg, min_count)
    for i in np.flatnonzero(out["flip"]):
        eng.negate_normals(int(i))
    eng.reset_history()
    out.update(pos=pos, neg=neg, counts=np.asarray(counts).copy())
    return out


def init_from_clouds(eng, frames, xyz_list, radius, tau, max_nn=64, edges=None, hypotheses=10000, seed=0, edge_sim=0.9, mutual=True, ratio=1.0,
                     min_count=3, root=0, refine=True, keypoints=None):
    """Initial poses of a multiview problem from the clouds alone: Engine.fpfh(device=True) of every frame of `frames` -> ONE
    Engine.coarse_pairs over `edges` (pairs (i, j) of positions in `frames`; default: all i < j; seeds[e] = seed + e) -> with `refine`,
    closedform_point_to_point over each edge's inliers in ascending pair order (when there are at least 3) -> poses_from_pairs over the
    inlier counts.  xyz_list: the stored clouds of the frames as numpy arrays.
    keypoints: None, or a dict(salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5, mode="both"): the
    descriptors are still computed on the FULL clouds, Engine.iss_keypoints selects rows of every frame, and only the selected rows are
    matched.  mode "both": every edge matches the keypoints of its two frames.  mode "src": the keypoints of the source against every
    point of the destination (2 K sets: the keypoints, then the full clouds; edge (i, j) becomes (i, K + j)), which does not depend on
    the two views selecting the same points.  The pair indices of coarse_pairs_fetch then refer to the matched rows, and the refinement
    uses those rows.
    -> dict(poses (K,4,4), edges (E,2), records = per edge dict(pairs, accepted, inliers, best, pose, refined), parent, parent_edge,
    component, components; with keypoints also keypoints = the index array of every frame)."""
    import torch
    K = len(frames)
    if len(xyz_list) != K:
        raise ValueError("xyz_list must hold one cloud per frame")
    if edges is None:
        edges = [(i, j) for i in range(K) for j in range(i + 1, K)]
    edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
    clouds = [np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3) for x in xyz_list]
    descs = [eng.fpfh(f, radius, max_nn, device=True)["desc"] for f in frames]
    for d, x in zip(descs, clouds):
        if d.shape[0] != len(x):
            raise ValueError("xyz_list does not hold the clouds of the frames")
    kp_idx, set_dst = None, edges[:, 1]
    src_rows = dst_rows = clouds   # the rows an edge's pair indices refer to, per frame
    if keypoints is not None:
        kp = dict(keypoints)
        mode = kp.pop("mode", "both")
        if mode not in ("both", "src"):
            raise ValueError("keypoints['mode'] must be 'both' or 'src'")
        kp_idx = [eng.iss_keypoints(f, **kp)["idx"] for f in frames]
        sel = [torch.from_numpy(ix.astype(np.int64)).to(d.device) for ix, d in zip(kp_idx, descs)]
        kp_descs = [d.index_select(0, t) for d, t in zip(descs, sel)]
        src_rows = [np.ascontiguousarray(x[ix]) for x, ix in zip(clouds, kp_idx)]
        if mode == "both":
            descs, dst_rows, clouds_in = kp_descs, src_rows, src_rows
        else:
            descs, clouds_in, set_dst = kp_descs + descs, src_rows + clouds, (edges[:, 1] + K).astype(np.int32)
    else:
        clouds_in = clouds
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in clouds_in])]).astype(np.int64)
    desc = torch.cat(descs, 0) if K else torch.zeros((0, 33), dtype=torch.float64, device=torch.device("cuda", eng.device))
    xyz = np.ascontiguousarray(np.concatenate(clouds_in, 0)) if K else np.zeros((0, 3))
    res = eng.coarse_pairs(desc, xyz, offsets, edges[:, 0], set_dst, seed, mutual=mutual, ratio=ratio, hypotheses=hypotheses, tau=tau, edge_sim=edge_sim)
    records, used = [], []
    for e, (i, j) in enumerate(edges):
        rec = {"pairs": int(res["pairs"][e]), "accepted": int(res["accepted"][e]), "inliers": int(res["count"][e]), "best": int(res["best"][e]),
               "pose": res["pose"][e].copy(), "refined": res["pose"][e].copy()}
        if refine and rec["inliers"] >= 3:
            pr, fl = eng.coarse_pairs_fetch(e)
            keep = fl != 0
            rec["refined"] = closedform_point_to_point(src_rows[i][pr[keep, 0]], dst_rows[j][pr[keep, 1]])
        records.append(rec)
        used.append(rec["refined"] if refine else rec["pose"])
    tree = poses_from_pairs(K, edges[:, 0], edges[:, 1], res["count"], np.array(used).reshape(-1, 4, 4), min_count, root)
    tree.update(edges=edges, records=records)
    if kp_idx is not None:
        tree["keypoints"] = kp_idx
    return tree


def lm_solve_host(n_frames, src, dst, poses, fixed, param, eval_callback, max_iterations=50):
    """mvicp_lm_solve with a Python evaluator: eval_callback(poses(K,4,4)) -> blocks (E,91).  Host only."""
    lib = load_library()
    src = np.ascontiguousarray(src, dtype=np.int32)
    dst = np.ascontiguousarray(dst, dtype=np.int32)
    E = len(src)
    P = poses_to_c(poses)
    fx = np.ascontiguousarray(fixed, dtype=np.uint8).copy()
    err = []

    def _cb(_user, p_ptr, b_ptr):
        try:
            pp = np.ctypeslib.as_array(p_ptr, shape=(n_frames, 16)).copy()
            blocks = np.asarray(eval_callback(poses_from_c(pp)), dtype=np.float64).reshape(E, EDGE_BLOCK)
            np.ctypeslib.as_array(b_ptr, shape=(E, EDGE_BLOCK))[:] = blocks
            return 0
        except Exception as ex:  # pragma: no cover - surfaced below
            err.append(ex)
            return -1

    sm = Summary()
    cb = EVAL_FN(_cb)
    st = lib.mvicp_lm_solve(n_frames, E, _ip(src), _ip(dst), _dp(P), fx.ctypes.data_as(C.POINTER(C.c_ubyte)), param, max_iterations, cb, None, C.byref(sm))
    if err:
        raise err[0]
    _check(lib, st)
    return poses_from_c(P), sm.as_dict()


class Engine:
    """One GPU context.  Mirrors the reference loop: set_frames -> set_graph -> (correspond -> optimize)*."""

    def __init__(self, device=0, rank=0, world=1):
        self.lib = load_library()
        h = C.c_void_p()
        self.device = device
        _check(self.lib, self.lib.mvicp_create(device, C.byref(h)))
        self.h = h
        self.n_frames = 0
        self.E = 0
        self.rank, self.world = rank, world
        if world > 1:
            _check(self.lib, self.lib.mvicp_set_shard(self.h, rank, world))

    def close(self):
        if self.h:
            self.lib.mvicp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- uploads
    def set_frames(self, pts_list, nor_list=None):
        self.n_frames = len(pts_list)
        _check(self.lib, self.lib.mvicp_set_num_frames(self.h, self.n_frames))
        self.npts = []
        for i, p in enumerate(pts_list):
            p = np.ascontiguousarray(p, dtype=np.float64)
            n = None if nor_list is None or nor_list[i] is None else np.ascontiguousarray(nor_list[i], dtype=np.float64)
            _check(self.lib, self.lib.mvicp_set_frame(self.h, i, _dp(p), _dp(n) if n is not None else None, len(p)))
            self.npts.append(len(p))

    def set_frame(self, frame, pts, nor=None):
        """Re-upload ONE cloud (before set_graph): mvicp_set_frame."""
        p = np.ascontiguousarray(pts, dtype=np.float64)
        n = None if nor is None else np.ascontiguousarray(nor, dtype=np.float64)
        _check(self.lib, self.lib.mvicp_set_frame(self.h, frame, _dp(p), _dp(n) if n is not None else None, len(p)))
        self.npts[frame] = len(p)

    def set_frame_device(self, frame, xyz, nor=None):
        """Upload ONE cloud that is already on the GPU (torch tensors, n x 3 float64): mvicp_set_frame_device.  The structures are
        built on the GPU; the tensors may be reused once this returns."""
        n = check_device_cloud(xyz, self.device)
        if nor is not None:
            check_device_cloud(nor, self.device, n, "nor")
        import torch
        torch.cuda.current_stream(xyz.device).synchronize()   # the call's contract: the arrays are fully written
        p = C.c_void_p(xyz.data_ptr()) if n else None
        q = C.c_void_p(nor.data_ptr()) if nor is not None and n else None
        _check(self.lib, self.lib.mvicp_set_frame_device(self.h, frame, p, q, n))
        self.npts[frame] = n

    def set_frames_device(self, xyz_list, nor_list=None):
        for i, t in enumerate(xyz_list):   # (every tensor is checked before the frames are reset)
            check_device_cloud(t, self.device)
            if nor_list is not None and nor_list[i] is not None:
                check_device_cloud(nor_list[i], self.device, int(t.shape[0]), "nor")
        self.n_frames = len(xyz_list)
        _check(self.lib, self.lib.mvicp_set_num_frames(self.h, self.n_frames))
        self.npts = [0] * self.n_frames
        for i, t in enumerate(xyz_list):
            self.set_frame_device(i, t, None if nor_list is None else nor_list[i])

    def get_structure(self, frame, name):
        """One per-cloud structure array as bytes (np.uint8), "scalars" / "build_ms" as float64: mvicp_get_structure."""
        nb = _check(self.lib, self.lib.mvicp_get_structure(self.h, frame, name.encode(), None, 0))
        buf = np.zeros(nb, dtype=np.uint8)
        _check(self.lib, self.lib.mvicp_get_structure(self.h, frame, name.encode(), buf.ctypes.data_as(C.c_void_p), nb))
        return buf.view(np.float64) if name in ("scalars", "build_ms") else buf

    def recompute_normals(self, frame, k=10, want_knn=False):
        n = self.npts[frame]
        nrm = np.zeros((n, 3), dtype=np.float64)
        knn = np.zeros((n, k), dtype=np.int32) if want_knn else None
        _check(self.lib, self.lib.mvicp_recompute_normals(self.h, frame, k, _dp(nrm), _ip(knn) if want_knn else None))
        return (nrm, knn) if want_knn else nrm

    def set_graph(self, src, dst):
        self.src = np.ascontiguousarray(src, dtype=np.int32)
        self.dst = np.ascontiguousarray(dst, dtype=np.int32)
        self.E = len(self.src)
        _check(self.lib, self.lib.mvicp_set_graph(self.h, self.E, _ip(self.src), _ip(self.dst)))

    def reset_history(self):
        """New registration on the same clouds / graph: the next correspond() behaves like the first one after set_graph()."""
        _check(self.lib, self.lib.mvicp_reset_history(self.h))

    def comm_init(self, unique_id, librccl_path=None):
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        path = librccl_path.encode() if librccl_path else None
        _check(self.lib, self.lib.mvicp_comm_init(self.h, path, C.cast(buf, C.c_void_p), self.rank, self.world))

    def comm_nranks(self):
        """ranks of the RCCL communicator as RCCL reports them (0: none)."""
        return int(self.lib.mvicp_comm_nranks(self.h))

    def comm_set_callback(self, allreduce):
        """allreduce(numpy float64 array) must sum it in place over all ranks (host-staged exchange, no RCCL)."""
        def _cb(_user, ptr, n):
            try:
                allreduce(np.ctypeslib.as_array(ptr, shape=(n,)))
                return 0
            except Exception:
                return -1
        self._ar_cb = ALLREDUCE_FN(_cb)   # keep alive
        _check(self.lib, self.lib.mvicp_comm_set_callback(self.h, self._ar_cb, None))

    @staticmethod
    def comm_unique_id(librccl_path=None):
        lib = load_library()
        buf = (C.c_char * 128)()
        path = librccl_path.encode() if librccl_path else None
        _check(lib, lib.mvicp_comm_unique_id(path, C.cast(buf, C.c_void_p)))
        return bytes(buf)

    # ---- S1
    def _round_buffers(self, K):
        """Per-engine staging buffers + their ctypes pointers for the two per-round calls (building numpy arrays and ctypes pointers
        anew costs ~10 us per call — a few per cent of a converged cfg4 round).  Results are handed back as copies."""
        b = getattr(self, "_rb", None)
        if b is None or b["K"] != K or b["E"] != self.E:
            P = np.zeros((K, 16)); fx = np.zeros(K, dtype=np.uint8)
            counts = np.zeros(self.E, dtype=np.int32); weights = np.zeros(self.E, dtype=np.float32)
            sm = Summary()
            b = {"K": K, "E": self.E, "P": P, "P44": P.reshape(K, 4, 4), "fx": fx, "counts": counts, "weights": weights, "sm": sm,
                 "pP": _dp(P), "pfx": fx.ctypes.data_as(C.POINTER(C.c_ubyte)), "pc": _ip(counts), "pw": weights.ctypes.data_as(C.POINTER(C.c_float)),
                 "psm": C.byref(sm)}
            self._rb = b
        return b

    def correspond(self, poses, fixed, thresh, nn_method=NN_AUTO):
        b = self._round_buffers(len(poses))
        np.copyto(b["P44"], np.transpose(np.asarray(poses, dtype=np.float64), (0, 2, 1)))   # 4x4 row-major -> column-major (Eigen)
        b["fx"][:] = fixed
        _check(self.lib, self.lib.mvicp_correspond(self.h, b["pP"], b["pfx"], np.float32(thresh), nn_method, b["pc"], b["pw"]))
        self.counts = b["counts"].copy()
        return self.counts, b["weights"].copy()

    # ---- the per-round calls without the (K,4,4) <-> column-major conversions: the caller keeps the poses in the engine's own K x 16
    # buffer (Eigen's layout) between the calls, like a C++ driver does.  bench.py's timed loop uses these.
    def round_state(self, K, fixed):
        """-> dict with "P" (K x 16 column-major poses, in/out), "counts", "weights", "sm" (the Summary struct of the last optimize_raw)."""
        b = self._round_buffers(K)
        b["fx"][:] = fixed
        return b

    def correspond_raw(self, thresh, nn_method=NN_AUTO):
        b = self._rb
        _check(self.lib, self.lib.mvicp_correspond(self.h, b["pP"], b["pfx"], thresh, nn_method, b["pc"], b["pw"]))

    def optimize_raw(self, param, point_to_plane, robust, max_iterations=50):
        b = self._rb
        _check(self.lib, self.lib.mvicp_optimize(self.h, b["pP"], b["pfx"], param, int(point_to_plane), int(robust), max_iterations, b["psm"]))
        return b["sm"]

    def get_correspondences(self, edge):
        cap = self.npts[self.src[edge]]
        first = np.zeros(cap, dtype=np.int32)
        second = np.zeros(cap, dtype=np.int32)
        dist = np.zeros(cap, dtype=np.float64)
        n = _check(self.lib, self.lib.mvicp_get_correspondences(self.h, edge, cap, _ip(first), _ip(second), _dp(dist)))
        return first[:n].copy(), second[:n].copy(), dist[:n].copy()

    CORR_DTYPE = np.dtype([("first", np.int32), ("second", np.int32), ("dist", np.float64)])   # struct Correspondance (include/frame.h:18-22)

    def map_correspondences(self, copy=True):
        """ALL lists of the last correspond() in the reference's layout: (triples, offsets) — a structured array of {first, second, dist}
        and E + 1 positions; edge e = triples[offsets[e]:offsets[e + 1]], ascending `first`.  copy=False returns a VIEW of the library's
        pinned buffer, valid until the next correspond() / set_correspondences() on this engine."""
        tp, op = C.c_void_p(), C.POINTER(C.c_longlong)()
        _check(self.lib, self.lib.mvicp_map_correspondences(self.h, C.byref(tp), C.byref(op)))
        off = np.ctypeslib.as_array(op, shape=(self.E + 1,)).copy()
        total = int(off[-1])
        if total == 0:
            return np.zeros(0, dtype=self.CORR_DTYPE), off
        buf = (C.c_char * (16 * total)).from_address(tp.value)
        t = np.frombuffer(buf, dtype=self.CORR_DTYPE, count=total)
        return (t.copy() if copy else t), off

    def map_correspondences_async(self):
        """mvicp_map_correspondences_async: VIEWS (triples, offsets) of the library's pinned buffer; edge e's bytes are defined after wait_correspondences(e)."""
        tp, op = C.c_void_p(), C.POINTER(C.c_longlong)()
        _check(self.lib, self.lib.mvicp_map_correspondences_async(self.h, C.byref(tp), C.byref(op)))
        off = np.ctypeslib.as_array(op, shape=(self.E + 1,)).copy()
        total = int(off[-1])
        if total == 0:
            return np.zeros(0, dtype=self.CORR_DTYPE), off
        buf = (C.c_char * (16 * total)).from_address(tp.value)
        return np.frombuffer(buf, dtype=self.CORR_DTYPE, count=total), off

    def wait_correspondences(self, edge):
        _check(self.lib, self.lib.mvicp_wait_correspondences(self.h, int(edge)))

    def correspondence_epochs(self):
        """Per-edge change counters of the lists (mvicp_correspondence_epochs): an edge whose list is provably last search's keeps its epoch."""
        ep = C.POINTER(C.c_ulonglong)()
        _check(self.lib, self.lib.mvicp_correspondence_epochs(self.h, C.byref(ep)))
        return np.ctypeslib.as_array(ep, shape=(self.E,)).copy()

    def set_correspondences(self, edge, first, second, weight=0.0):
        first = np.ascontiguousarray(first, dtype=np.int32)
        second = np.ascontiguousarray(second, dtype=np.int32)
        _check(self.lib, self.lib.mvicp_set_correspondences(self.h, edge, len(first), _ip(first), _ip(second), np.float32(weight)))

    def overlap(self, poses, thresh, max_samples=4096):
        """mvicp_overlap: census of ALL ordered frame pairs at `poses` -> dict(samples (K), hits (K,K), sumq (K,K) int64, q_exp,
        fraction = hits / samples[:, None], mean_d2 = sumq / max(hits, 1) * 2^-q_exp).  Needs no graph; history-neutral."""
        P = poses_to_c(poses)
        K = len(P)
        samples = np.zeros(K, dtype=np.int32); hits = np.zeros((K, K), dtype=np.int32); sumq = np.zeros((K, K), dtype=np.int64)
        q = C.c_int(0)
        _check(self.lib, self.lib.mvicp_overlap(self.h, _dp(P), np.float32(thresh), int(max_samples), _ip(samples), _ip(hits),
                                                sumq.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(q)))
        fraction = hits / np.maximum(samples, 1)[:, None].astype(np.float64)
        mean_d2 = np.ldexp(sumq / np.maximum(hits, 1).astype(np.float64), -q.value)
        return {"samples": samples, "hits": hits, "sumq": sumq, "q_exp": int(q.value), "fraction": fraction, "mean_d2": mean_d2}

    def _result_arrays(self, device):
        """What the fetch half of a stage needs -> (mk, ptr, ready, f64, i32, i64, u8): mk(shape, dtype) makes a result array (numpy zeros,
        or with device=True an uninitialised torch tensor on the engine's GPU), ptr(a) is its pointer or None for an absent or empty
        array, ready() is called once between the last mk and the fetch (the allocations are the caller's; the library fills them on its
        own stream and waits), and the rest are the dtypes for mk."""
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            return (lambda shape, dt: torch.empty(shape, dtype=dt, device=dev),
                    lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None,
                    lambda: torch.cuda.synchronize(dev), torch.float64, torch.int32, torch.int64, torch.uint8)
        return (lambda shape, dt: np.zeros(shape, dtype=dt),
                lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None,
                lambda: None, np.float64, np.int32, np.int64, np.uint8)

    def _fetch_kept(self, fetch, kept, device, label=False):
        """The kept rows of a selection -> dict(xyz (kept,3), nrm (kept,3) or None, idx (kept,) int32, and with label=True label (kept,)
        int32).  fetch(xyz, nrm, idx, label) is the stage's fetch call with the row pointers in these places.  The selection carries
        normals iff its frame had stored normals when it ran, and the C calls have no record that says so: asking for them answers it -- a
        refusal is MVICP_ERR_STATE and writes nothing; with no rows nothing is written either way, so any non-NULL pointer asks."""
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        out = {"xyz": mk((kept, 3), f64), "nrm": mk((kept, 3), f64), "idx": mk((kept,), i32)}
        if label:
            out["label"] = mk((kept,), i32)
        ready()
        st = fetch(None, ptr(out["nrm"]) if kept else C.c_void_p(8), None, None)
        if st == -3:   # (MVICP_ERR_STATE: no normals -- or no result at all, which the fetch below then reports)
            out["nrm"] = None
        else:
            _check(self.lib, st)
        _check(self.lib, fetch(ptr(out["xyz"]), None, ptr(out["idx"]), ptr(out.get("label"))))
        return out

    def voxel_grid(self, voxel, frames=None, poses=None, device=False):
        """mvicp_voxel_grid + mvicp_voxel_fetch: the points of `frames` (a list of distinct frame indices; None = all), at `poses` ((K,4,4);
        None = as stored), reduced to one point per voxel of edge `voxel` -> dict(xyz (m,3), nrm (m,3) or None, cnt (m,) int32), rows in
        ascending voxel key.  device=True: torch tensors on the engine's GPU (ready for set_frame_device) instead of numpy arrays.
        Needs no graph; history-neutral."""
        if frames is None:
            n_sel, fp = 0, None
        else:
            fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
            n_sel = len(fr)
            fr = np.concatenate([fr, np.zeros(1, dtype=np.int32)])   # (never a NULL pointer for an empty selection: NULL means "all")
            fp = _ip(fr)
        P = None if poses is None else poses_to_c(poses)
        hn = C.c_int(0)
        st = self.lib.mvicp_voxel_grid(self.h, n_sel, fp, _dp(P) if P is not None else None, float(voxel), C.byref(hn))
        m = int(_check(self.lib, st))
        has_nrm = bool(hn.value)
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        xyz, nrm, cnt = mk((m, 3), f64), (mk((m, 3), f64) if has_nrm else None), mk((m,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_voxel_fetch(self.h, m, ptr(xyz), ptr(nrm), ptr(cnt)))
        return {"xyz": xyz, "nrm": nrm, "cnt": cnt}

    def outlier_filter(self, frame, k=16, std_ratio=2.0, radius=0.0, device=False):
        """mvicp_outlier_filter + mvicp_outlier_fetch on the stored cloud of `frame`: the statistical rule (mean distance to the k nearest
        neighbours against mean + std_ratio * sigma over the cloud; std_ratio < 0: off) and the radius rule (at least k neighbours within
        `radius`; radius <= 0: off) -> dict(xyz (kept,3), nrm (kept,3) or None, idx (kept,) int32 original indices ascending, mdist (n,),
        kd2 (n,), stats).  device=True: torch tensors on the engine's GPU (xyz / nrm ready for set_frame_device) instead of numpy arrays.
        Needs no graph; history-neutral."""
        S = OutlierStats()
        kept = int(_check(self.lib, self.lib.mvicp_outlier_filter(self.h, int(frame), int(k), float(std_ratio), float(radius), C.byref(S))))
        n = int(S.n)
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        mdist, kd2 = mk((n,), f64), mk((n,), f64)
        # (_fetch_kept calls this twice: first with nrm alone, to learn whether normals come along, then with the rows and nrm = None.  The
        # per-point arrays mdist / kd2 are copied once, by the second call)
        out = self._fetch_kept(lambda xyz, nrm, idx, label: self.lib.mvicp_outlier_fetch(self.h, kept, xyz, nrm, idx, n, None if nrm else ptr(mdist),
                                                                                          None if nrm else ptr(kd2)), kept, device)
        out.update(mdist=mdist, kd2=kd2, stats=S.as_dict())
        return out

    def cluster(self, frame, radius, min_pts=4, device=False):
        """mvicp_cluster + mvicp_cluster_fetch on the stored cloud of `frame`: DBSCAN with the strict radius predicate of knn_search, the
        point itself counting towards min_pts, border points joining the cluster of their first core neighbour in the order (d2, index),
        clusters numbered by their smallest core index -> dict(label (n,) int32 with -1 = noise, core (n,) uint8, size (C,) int32,
        stats).  min_pts = 1: plain Euclidean cluster extraction.  device=True: torch tensors on the engine's GPU instead of numpy arrays.
        Needs no graph; history-neutral."""
        S = ClusterStats()
        nc = int(_check(self.lib, self.lib.mvicp_cluster(self.h, int(frame), float(radius), int(min_pts), C.byref(S))))
        n = int(S.n)
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        label, core, size = mk((n,), i32), mk((n,), u8), mk((nc,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_cluster_fetch(self.h, n, ptr(label), ptr(core), nc, ptr(size)))
        return {"label": label, "core": core, "size": size, "stats": S.as_dict()}

    def cluster_select(self, min_size=0, max_clusters=0, device=False):
        """mvicp_cluster_select + mvicp_cluster_fetch_kept on the last cluster() result: the points of the clusters that cluster_keep_rule
        keeps (noise always goes), in ascending original index -> dict(xyz (kept,3), nrm (kept,3) or None, idx (kept,) int32, label (kept,)
        int32, kept).  device=True: torch tensors on the engine's GPU (xyz / nrm ready for set_frame_device)."""
        kept = int(_check(self.lib, self.lib.mvicp_cluster_select(self.h, int(min_size), int(max_clusters))))
        out = self._fetch_kept(lambda xyz, nrm, idx, label: self.lib.mvicp_cluster_fetch_kept(self.h, kept, xyz, nrm, idx, label), kept, device, label=True)
        out["kept"] = kept
        return out

    def segment_plane(self, frame, tau, hypotheses=1024, seed=0, axis=None, cos_min=0.0, refine=True, device=False):
        """mvicp_segment_plane + mvicp_plane_fetch on the stored cloud of `frame`: the plane with the most points within tau among
        `hypotheses` three-point samples (the generator of consensus; the lowest h among equals), with axis (3,) only planes whose normal
        has |cos| >= cos_min to it, refitted over its inliers through exact integer moments (refine) -> dict(the record's fields: best,
        count, accepted, refit, count_refined, b, q, n, has_normals, normal, point, d, hyp_normal, hyp_point; counts (hypotheses,) int32
        with -1 = rejected; flags (n,) uint8).  device=True: counts / flags as torch tensors on the engine's GPU.  Needs no graph and no
        structure; history-neutral."""
        R = PlaneResult()
        ax = None if axis is None else np.ascontiguousarray(axis, dtype=np.float64).reshape(3)
        _check(self.lib, self.lib.mvicp_segment_plane(self.h, int(frame), int(hypotheses), int(seed) & (2 ** 64 - 1), float(tau), _dp(ax) if ax is not None else None,
                                                      float(cos_min), 1 if refine else 0, C.byref(R)))
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        counts, flags = mk((int(hypotheses),), i32), mk((int(R.n),), u8)
        ready()
        _check(self.lib, self.lib.mvicp_plane_fetch(self.h, int(hypotheses), ptr(counts), int(R.n), ptr(flags)))
        out = R.as_dict()
        out.update(counts=counts, flags=flags)
        return out

    def plane_select(self, inliers=True, device=False):
        """mvicp_plane_select + mvicp_plane_fetch_kept on the last segment_plane() result: the points of the plane (inliers) or the rest,
        in ascending original index -> dict(xyz (kept,3), nrm (kept,3) or None, idx (kept,) int32, kept).  device=True: torch tensors on
        the engine's GPU (xyz / nrm ready for set_frame_device)."""
        kept = int(_check(self.lib, self.lib.mvicp_plane_select(self.h, 1 if inliers else 0)))
        out = self._fetch_kept(lambda xyz, nrm, idx, label: self.lib.mvicp_plane_fetch_kept(self.h, kept, xyz, nrm, idx), kept, device)
        out["kept"] = kept
        return out

    def boundary(self, frame, max_nn=30, radius=0.0, cos_gap=-0.5, source=0, device=False):
        """mvicp_boundary + mvicp_boundary_fetch on the stored cloud of `frame`: a point is flagged when, in its tangent plane (normals of
        `source`: 0 the frame's stored ones, 1 the last estimate_normals / fit_normals of this frame), the directions to the neighbours of
        its row (the max_nn nearest, within `radius` if > 0) leave a gap of at least acos(cos_gap) -> dict(flag (n,) uint8, open (n,) int32
        = the directions that look into such a gap, valid (n,) int32 = the directions of the row, used (n,) int32 = the row's length,
        boundary = the number flagged).  device=True: torch tensors on the engine's GPU.  Leaves its search as the last neighbour search;
        needs no graph; otherwise history-neutral."""
        flagged = int(_check(self.lib, self.lib.mvicp_boundary(self.h, int(frame), int(source), int(max_nn), float(radius), float(cos_gap))))
        n = int(self.npts[frame])
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        flag, opn, valid, used = mk((n,), u8), mk((n,), i32), mk((n,), i32), mk((n,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_boundary_fetch(self.h, n, ptr(flag), ptr(opn), ptr(valid), ptr(used)))
        return {"flag": flag, "open": opn, "valid": valid, "used": used, "boundary": flagged}

    def boundary_select(self, boundary=True, device=False):
        """mvicp_boundary_select + mvicp_boundary_fetch_kept on the last boundary() result: the flagged points (boundary) or the rest, in
        ascending original index -> dict(xyz (kept,3), nrm (kept,3) or None, idx (kept,) int32, kept).  device=True: torch tensors on
        the engine's GPU (xyz / nrm ready for set_frame_device)."""
        kept = int(_check(self.lib, self.lib.mvicp_boundary_select(self.h, 1 if boundary else 0)))
        out = self._fetch_kept(lambda xyz, nrm, idx, label: self.lib.mvicp_boundary_fetch_kept(self.h, kept, xyz, nrm, idx), kept, device)
        out["kept"] = kept
        return out

    def reject_correspondences(self, dst_masks, src_masks=None):
        """Drops from every list this engine owns the pairs that end on a flagged point: per owned edge e = (s, d) get_correspondences(e),
        reject_by_mask with src_masks[s] / dst_masks[d] (sequences indexed by frame; an entry, or src_masks itself, may be None), then
        set_correspondences(e, kept, weight = the weight the last correspond() returned for e).  -> (E,) int32, the pairs dropped per edge
        (0 for edges of other ranks).  The default rejects on the target side only (Rusinkiewicz & Levoy 2001, section 3.4, for partial
        overlap; rejecting on the source side as well did not help on the project's test pair).
        A host composition of existing calls, with their consequences: the lists are EXPLICIT until the next correspond(); their stored
        distances read 0; installing them gives every owned edge a new epoch, drops the evaluation the search queued ahead and invalidates
        the temporal NN cache, so the next search runs like a first search.  On a sharded context the header's rule for explicit lists
        applies: set the option "spec_eval" to 0 on every rank."""
        rb = getattr(self, "_rb", None)
        if rb is None:
            raise MvicpError("reject_correspondences needs a correspond() before it")
        weights = rb["weights"]
        owner = edge_owner([self.npts[s] for s in self.src], self.world) if self.world > 1 else np.zeros(self.E, dtype=np.int32)
        dropped = np.zeros(self.E, dtype=np.int32)
        for e in range(self.E):
            if owner[e] != self.rank:
                continue
            s, d = int(self.src[e]), int(self.dst[e])
            first, second, _ = self.get_correspondences(e)
            kf, ks = reject_by_mask(first, second, None if src_masks is None else src_masks[s], None if dst_masks is None else dst_masks[d])
            self.set_correspondences(e, kf, ks, weights[e])
            dropped[e] = len(first) - len(kf)
        return dropped

    def set_reject_mask(self, frame, mask, roles=REJECT_AS_TARGET):
        """mvicp_set_reject_mask: `mask` (one byte per point of `frame` in original order, nonzero = reject: a numpy array, a uint8 torch
        tensor on the engine's GPU, or None = clear) is applied INSIDE every later correspond() -- a pair whose target (REJECT_AS_TARGET),
        source (REJECT_AS_SOURCE) or either end (both, or-ed) is flagged is dropped, and counts, lists, distances and the weight are those
        of the kept pairs.  Unlike reject_correspondences the lists stay searched lists: nothing crosses the bus and the temporal cache,
        the in-place upkeep and the queued evaluations keep working.  Note the weight: the median over the KEPT pairs, where
        reject_correspondences keeps the unfiltered list's."""
        if mask is None or not 0 <= int(frame) < len(self.npts):   # (a frame out of range: the library refuses it)
            mask = None if mask is None else C.cast(C.create_string_buffer(8), C.c_void_p)
            _check(self.lib, self.lib.mvicp_set_reject_mask(self.h, int(frame), mask, int(roles)))
            return
        n = int(self.npts[int(frame)])
        if isinstance(mask, np.ndarray) or not hasattr(mask, "data_ptr"):
            a = np.asarray(mask).reshape(-1)
            keep = np.ascontiguousarray(a) if a.dtype == np.uint8 else np.ascontiguousarray(a != 0, dtype=np.uint8)   # (uint8 bytes go in as they are)
            if len(keep) != n:
                raise MvicpError(f"set_reject_mask: {len(keep)} flags for the {n} points of frame {frame}")
            p = keep.ctypes.data_as(C.c_void_p) if n else C.cast(C.create_string_buffer(8), C.c_void_p)   # (never NULL: NULL clears)
        else:
            import torch
            if not mask.is_cuda or mask.dtype != torch.uint8 or (mask.device.index or 0) != self.device:
                raise MvicpError("set_reject_mask: a torch `mask` must be a uint8 tensor on the engine's GPU")
            keep = mask.contiguous().reshape(-1)
            if keep.shape[0] != n:
                raise MvicpError(f"set_reject_mask: {keep.shape[0]} flags for the {n} points of frame {frame}")
            torch.cuda.synchronize(keep.device)   # (a device array must be fully written when the call is made)
            p = C.c_void_p(keep.data_ptr()) if n else C.cast(C.create_string_buffer(8), C.c_void_p)
        _check(self.lib, self.lib.mvicp_set_reject_mask(self.h, int(frame), p, int(roles)))

    def adopt_boundary_mask(self, roles=REJECT_AS_TARGET):
        """mvicp_boundary_adopt: the flags of the last boundary() become that frame's reject mask without leaving the device."""
        _check(self.lib, self.lib.mvicp_boundary_adopt(self.h, int(roles)))

    def reject_mask(self, frame):
        """mvicp_get_reject_mask -> (mask (n,) uint8 in original order or None when the frame has none, roles)."""
        roles = C.c_int(0)
        n = int(_check(self.lib, self.lib.mvicp_get_reject_mask(self.h, int(frame), None, 0, C.byref(roles))))
        if roles.value == 0:
            return None, 0
        out = np.zeros(n, dtype=np.uint8)
        _check(self.lib, self.lib.mvicp_get_reject_mask(self.h, int(frame), out.ctypes.data_as(C.c_void_p) if n else None, n, C.byref(roles)))
        return out, int(roles.value)

    def knn_search(self, frame, queries=None, k=8, radius=0.0, device=False):
        """mvicp_knn_search + mvicp_knn_fetch on the stored cloud of `frame`: per query the candidates (every point, or with radius > 0 the
        points with sqrt(d2) < radius) in the order (d2, original index).  1 <= k <= 64: the first k of them -> dict(cnt (m,) int32,
        off (m+1,) int64 = i k, idx (m,k) int32 padded with -1, d2 (m,k) padded with +inf, total).  k = 0 (needs radius > 0): all of them in
        CSR form -> idx / d2 flat with off[m] entries.  queries: (m,3) numpy array, a float64 torch tensor on the engine's GPU, or None =
        the cloud's own points (row i = point i).  device=True: torch tensors on the engine's GPU instead of numpy arrays.
        Needs no graph; history-neutral."""
        keep = None
        if queries is None:
            qp, m = None, 0
        elif isinstance(queries, np.ndarray) or not hasattr(queries, "data_ptr"):
            keep = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
            m = len(keep)
            qp = keep.ctypes.data_as(C.c_void_p) if m else C.cast(C.create_string_buffer(24), C.c_void_p)   # (never NULL: NULL means self mode)
        else:
            import torch
            if not queries.is_cuda or queries.dtype != torch.float64 or (queries.device.index or 0) != self.device:
                raise MvicpError("knn_search: a torch `queries` must be a float64 tensor on the engine's GPU")
            keep = queries.contiguous().reshape(-1, 3)
            m = keep.shape[0]
            torch.cuda.synchronize(keep.device)   # (a device array must be fully written when the call is made)
            qp = C.c_void_p(keep.data_ptr()) if m else C.cast(C.create_string_buffer(24), C.c_void_p)
        total = int(_check(self.lib, self.lib.mvicp_knn_search(self.h, int(frame), qp, m, int(k), float(radius))))
        if queries is None:
            m = self.npts[int(frame)]
        k = int(k)
        entries = m * k if k else total
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        cnt, off, idx, d2 = mk((m,), i32), mk((m + 1,), i64), mk((entries,), i32), mk((entries,), f64)
        ready()
        _check(self.lib, self.lib.mvicp_knn_fetch(self.h, m, entries, ptr(cnt), ptr(off), ptr(idx), ptr(d2)))
        if k:
            idx, d2 = idx.reshape(m, k), d2.reshape(m, k)
        return {"cnt": cnt, "off": off, "idx": idx, "d2": d2, "total": total}

    def fpfh(self, frame, radius, max_nn=64, device=False):
        """mvicp_fpfh + mvicp_fpfh_fetch on the stored cloud and normals of `frame`: the 33-bin FPFH descriptor of every point over its
        max_nn nearest neighbours within `radius` -> dict(desc (n,33) float64, used (n,) int32 = neighbours that entered).  device=True:
        torch tensors on the engine's GPU instead of numpy arrays.  Afterwards the engine's last neighbour-search result is
        knn_search(frame, None, max_nn, radius).  Needs no graph; history-neutral."""
        n = int(_check(self.lib, self.lib.mvicp_fpfh(self.h, int(frame), float(radius), int(max_nn))))
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        desc, used = mk((n, 33), f64), mk((n,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_fpfh_fetch(self.h, n, ptr(desc), ptr(used)))
        return {"desc": desc, "used": used}

    def iss_keypoints(self, frame, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5, device=False):
        """mvicp_iss_keypoints + mvicp_iss_fetch on the stored cloud of `frame`: the ISS keypoints (Zhong 2009) -- points whose
        neighbourhood within `salient_radius` has eigenvalue ratios l2 / l1 < gamma21 and l3 / l2 < gamma32 and at least `min_neighbors`
        points, and whose l3 no neighbour within `non_max_radius` beats (the lowest index wins a tie) -> dict(idx (k,) int32 original
        indices ascending, xyz (k,3) the stored rows at idx, saliency (n,), cnt_salient (n,) int32, cnt_nms (n,) int32).  device=True:
        torch tensors on the engine's GPU instead of numpy arrays.  Needs no graph; history-neutral."""
        k = int(_check(self.lib, self.lib.mvicp_iss_keypoints(self.h, int(frame), float(salient_radius), float(non_max_radius), float(gamma21),
                                                              float(gamma32), int(min_neighbors))))
        n = self.npts[int(frame)]
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        idx, xyz = mk((k,), i32), mk((k, 3), f64)
        sal, cs, cn = mk((n,), f64), mk((n,), i32), mk((n,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_iss_fetch(self.h, k, ptr(idx), ptr(xyz), None, n, ptr(sal), ptr(cs), ptr(cn)))
        return {"idx": idx, "xyz": xyz, "saliency": sal, "cnt_salient": cs, "cnt_nms": cn}

    def estimate_normals(self, frame, max_nn=30, radius=0.0, viewpoint=None, device=False):
        """mvicp_estimate_normals + mvicp_normals_fetch on the stored cloud of `frame`: per point the direction of least variance of its
        max_nn nearest neighbours (radius > 0: within `radius`), turned towards `viewpoint` (3 numbers in the frame's local coordinates;
        None = the origin), and the surface variation -> dict(nrm (n,3) float64, curvature (n,) float64, used (n,) int32 = neighbours
        that entered; fewer than 3: a zero row).  device=True: torch tensors on the engine's GPU instead of numpy arrays.  The frame's
        own normals are untouched until adopt_normals().  Afterwards the engine's last neighbour-search result is
        knn_search(frame, None, max_nn, radius).  Needs no graph; history-neutral."""
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        n = int(_check(self.lib, self.lib.mvicp_estimate_normals(self.h, int(frame), int(max_nn), float(radius), _dp(vp) if vp is not None else None)))
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        nrm, curv, used = mk((n, 3), f64), mk((n,), f64), mk((n,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_normals_fetch(self.h, n, ptr(nrm), ptr(curv), ptr(used)))
        return {"nrm": nrm, "curvature": curv, "used": used}

    def fit_normals(self, frame, max_nn=16, radius=0.0, viewpoint=None, degree=3, device=False):
        """mvicp_fit_normals + mvicp_normals_fetch + mvicp_normals_fit_fetch on the stored cloud of `frame`: the normal of estimate_normals
        corrected by the slope of a height polynomial of `degree` 2 or 3 fitted over its tangent plane (an osculating jet) -> dict(nrm
        (n,3) float64, curvature (n,) float64 = the PCA surface variation, used (n,) int32, fitted (n,) uint8 = 1 where the row is the fit,
        0 where it kept the PCA estimate: fewer than 6 / 10 neighbours, or a refused factorisation).  device=True: torch tensors on the
        engine's GPU instead of numpy arrays.  The result takes the place of the last estimate_normals: adopt_normals() and
        orient_normals(source=1) act on it.  Afterwards the engine's last neighbour-search result is knn_search(frame, None, max_nn,
        radius).  Needs no graph; history-neutral."""
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        n = int(_check(self.lib, self.lib.mvicp_fit_normals(self.h, int(frame), int(max_nn), float(radius), _dp(vp) if vp is not None else None,
                                                            int(degree))))
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        nrm, curv, used, fitted = mk((n, 3), f64), mk((n,), f64), mk((n,), i32), mk((n,), u8)
        ready()
        _check(self.lib, self.lib.mvicp_normals_fetch(self.h, n, ptr(nrm), ptr(curv), ptr(used)))
        _check(self.lib, self.lib.mvicp_normals_fit_fetch(self.h, n, ptr(fitted)))
        return {"nrm": nrm, "curvature": curv, "used": used, "fitted": fitted}

    def smooth_points(self, frame, max_nn=30, radius=0.0, viewpoint=None, degree=2, max_shift=0.0, device=False):
        """mvicp_smooth_points + mvicp_smooth_fetch + the two normals fetches on the stored cloud of `frame`: every point moved onto the
        height polynomial of `degree` 2 or 3 fitted through its max_nn nearest neighbours, along its PCA normal (jet smoothing), and the
        mean and Gaussian curvature of that polynomial -> dict(xyz (n,3) float64 = the moved points, shift (n,) float64 = the signed
        distance moved along the PCA normal, moved (n,) uint8 = 0 where the row was not fitted or |shift| > max_shift > 0 (xyz is then the
        stored point), H, K (n,) float64 (H > 0 where the surface bends towards the normal; see principal_curvatures), and nrm, curvature,
        used, fitted exactly as fit_normals returns them).  device=True: torch tensors on the engine's GPU, ready for set_frame_device.
        The stored cloud is untouched.  The result takes the place of the last estimate_normals / fit_normals: adopt_normals() and
        orient_normals(source=1) act on its nrm.  Afterwards the engine's last neighbour-search result is knn_search(frame, None, max_nn,
        radius).  Needs no graph; history-neutral."""
        vp = None if viewpoint is None else np.ascontiguousarray(viewpoint, dtype=np.float64).reshape(3)
        n = int(_check(self.lib, self.lib.mvicp_smooth_points(self.h, int(frame), int(max_nn), float(radius), _dp(vp) if vp is not None else None,
                                                              int(degree), float(max_shift))))
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        nrm, curv, used, fitted = mk((n, 3), f64), mk((n,), f64), mk((n,), i32), mk((n,), u8)
        xyz, shift, moved, H, K = mk((n, 3), f64), mk((n,), f64), mk((n,), u8), mk((n,), f64), mk((n,), f64)
        ready()
        _check(self.lib, self.lib.mvicp_normals_fetch(self.h, n, ptr(nrm), ptr(curv), ptr(used)))
        _check(self.lib, self.lib.mvicp_normals_fit_fetch(self.h, n, ptr(fitted)))
        _check(self.lib, self.lib.mvicp_smooth_fetch(self.h, n, ptr(xyz), ptr(shift), ptr(moved), ptr(H), ptr(K)))
        return {"xyz": xyz, "nrm": nrm, "curvature": curv, "used": used, "fitted": fitted, "shift": shift, "moved": moved, "H": H, "K": K}

    def adopt_normals(self):
        """mvicp_normals_adopt: the frame of the last estimate_normals or fit_normals takes that result as its normals, as recompute_normals would
        leave them (lists that point into the frame are re-gathered, queued evaluations are voided)."""
        _check(self.lib, self.lib.mvicp_normals_adopt(self.h))

    def orient_normals(self, frame, k=10, radius=0.0, source=0, mode=ORIENT_ANCHOR, ref=None, device=False):
        """mvicp_orient_normals + mvicp_orient_fetch: the normals of `frame` (source 0: its stored ones, 1: those of the last
        estimate_normals of this frame) made consistent with each other along the maximum spanning forest of the graph of the k nearest
        neighbours (radius > 0: within `radius`) weighted by |N_i . N_j|; every tree's sign is its lowest point's (ORIENT_ANCHOR), or a
        majority vote towards the point `ref` (ORIENT_VIEWPOINT; None = the origin) or along the direction `ref` (ORIENT_DIRECTION)
        -> dict(nrm (n,3) float64, flip (n,) uint8, comp (n,) int32 = the lowest point of the tree, components).  device=True: torch
        tensors on the engine's GPU instead of numpy arrays.  The frame's own normals are untouched until adopt_orientation().
        Afterwards the engine's last neighbour-search result is knn_search(frame, None, k, radius).  Needs no graph; history-neutral."""
        rf = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64).reshape(3)
        comps = int(_check(self.lib, self.lib.mvicp_orient_normals(self.h, int(frame), int(source), int(k), float(radius), int(mode),
                                                                   _dp(rf) if rf is not None else None)))
        n = self.npts[int(frame)]
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        nrm, flip, comp = mk((n, 3), f64), mk((n,), u8), mk((n,), i32)
        ready()
        _check(self.lib, self.lib.mvicp_orient_fetch(self.h, n, ptr(nrm), ptr(flip), ptr(comp)))
        return {"nrm": nrm, "flip": flip, "comp": comp, "components": comps}

    def adopt_orientation(self):
        """mvicp_orient_adopt: the frame of the last orient_normals takes that result as its normals, with the side effects of adopt_normals."""
        _check(self.lib, self.lib.mvicp_orient_adopt(self.h))

    def normal_agreement(self, poses):
        """mvicp_normal_agreement at `poses` ((K,4,4)) over the lists the engine holds -> (pos (E,) int32, neg (E,) int32): per edge the pairs
        whose normals, rotated into the world, have a positive / a negative dot.  History-neutral."""
        P = poses_to_c(poses)
        E = self.E
        pos, neg = np.zeros(max(E, 1), dtype=np.int32), np.zeros(max(E, 1), dtype=np.int32)
        _check(self.lib, self.lib.mvicp_normal_agreement(self.h, _dp(P), _ip(pos), _ip(neg)))
        return pos[:E].copy(), neg[:E].copy()

    def negate_normals(self, frame):
        """mvicp_negate_normals: every stored normal of `frame` is negated, with the side effects of adopt_normals."""
        _check(self.lib, self.lib.mvicp_negate_normals(self.h, int(frame)))

    def _rows_operand(self, x, cols, what):
        """-> (the array kept alive, its pointer or None when empty, rows) for a (rows, cols) float64 numpy array or torch tensor on the engine's GPU"""
        if isinstance(x, np.ndarray) or not hasattr(x, "data_ptr"):
            keep = np.ascontiguousarray(x, dtype=np.float64)
            keep = keep.reshape(-1, cols) if cols else keep
            if keep.ndim != 2:
                raise MvicpError(f"{what} must be a matrix")
            return keep, (keep.ctypes.data_as(C.c_void_p) if keep.size else None), keep.shape[0]
        import torch
        if not x.is_cuda or x.dtype != torch.float64 or (x.device.index or 0) != self.device:
            raise MvicpError(f"a torch `{what}` must be a float64 tensor on the engine's GPU")
        keep = x.contiguous()
        keep = keep.reshape(-1, cols) if cols else keep
        if keep.dim() != 2:
            raise MvicpError(f"{what} must be a matrix")
        torch.cuda.synchronize(keep.device)   # (a device array must be fully written when the call is made)
        return keep, (C.c_void_p(keep.data_ptr()) if keep.numel() else None), int(keep.shape[0])

    def feature_match(self, a, b, device=False):
        """mvicp_feature_match + mvicp_feature_match_fetch: a (m, dim), b (n, dim), 1 <= dim <= 64, numpy arrays or float64 torch tensors
        on the engine's GPU.  Per row of a the two nearest rows of b in the order (dist, j), dist = the sequential fp64 sum of squared
        differences, and the reverse -> dict(fwd_idx (m,2) int32, fwd_d2 (m,2), bwd_idx (n,2) int32, bwd_d2 (n,2)), a missing entry
        padded with (-1, +inf).  device=True: torch tensors on the engine's GPU.  Needs no frame and no graph; history-neutral."""
        ka, pa, m = self._rows_operand(a, 0, "a")
        kb, pb, n = self._rows_operand(b, 0, "b")
        if ka.shape[1] != kb.shape[1]:
            raise MvicpError(f"a has {ka.shape[1]} columns, b {kb.shape[1]}")
        got = int(_check(self.lib, self.lib.mvicp_feature_match(self.h, pa, m, pb, n, int(ka.shape[1]))))
        assert got == m
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        fi, fd, bi, bd = mk((m, 2), i32), mk((m, 2), f64), mk((n, 2), i32), mk((n, 2), f64)
        ready()
        _check(self.lib, self.lib.mvicp_feature_match_fetch(self.h, m, n, ptr(fi), ptr(fd), ptr(bi), ptr(bd)))
        return {"fwd_idx": fi, "fwd_d2": fd, "bwd_idx": bi, "bwd_d2": bd}

    def consensus(self, P, Q, hypotheses, seed, tau, edge_sim=0.9):
        """mvicp_consensus + mvicp_consensus_fetch: P, Q (c, 3) index-aligned pairs src -> dst (numpy arrays or float64 torch tensors on
        the engine's GPU), `hypotheses` triangle-frame poses drawn from `seed`, each scored by its pairs within tau; edge_sim rejects
        triangles whose edge lengths differ by more than that factor -> dict(best, count, accepted, pose (4,4), counts (H,) int32 with
        -1 = rejected, flags (c,) uint8 = the winner's inliers).  Needs no frame and no graph; history-neutral."""
        kp, pp, c = self._rows_operand(P, 3, "P")
        kq, pq, cq = self._rows_operand(Q, 3, "Q")
        if c != cq:
            raise MvicpError(f"P has {c} rows, Q {cq}")
        res = ConsensusResult()
        _check(self.lib, self.lib.mvicp_consensus(self.h, pp, pq, c, int(hypotheses), int(seed) & (2 ** 64 - 1), float(tau), float(edge_sim), C.byref(res)))
        counts, flags = np.zeros(int(hypotheses), dtype=np.int32), np.zeros(c, dtype=np.uint8)
        _check(self.lib, self.lib.mvicp_consensus_fetch(self.h, len(counts), counts.ctypes.data_as(C.c_void_p), c, flags.ctypes.data_as(C.c_void_p)))
        return {"best": int(res.best), "count": int(res.count), "accepted": int(res.accepted), "pose": poses_from_c(np.array(res.pose[:]))[0],
                "counts": counts, "flags": flags}

    def coarse_pairs(self, desc, xyz, offsets, src, dst, seeds=None, mutual=True, ratio=1.0, hypotheses=10000, tau=None, edge_sim=0.9):
        """mvicp_coarse_pairs: for every edge (src[e], dst[e]) over the sets whose rows are offsets[s] .. offsets[s+1] of desc (total, dim)
        and xyz (total, 3) the chain feature_match -> match_pairs(mutual, ratio) -> gather -> consensus(hypotheses, seeds[e], tau, edge_sim)
        in one call, the same bytes as the chain of single calls.  desc / xyz: numpy arrays or float64 torch tensors on the engine's GPU.
        seeds: one per edge, or None / an int s for seeds[e] = s + e mod 2^64.
        -> dict(pairs, best, count, accepted: (E,) int32; pose (E,4,4)).  Needs no frame and no graph; history-neutral."""
        if tau is None:
            raise ValueError("coarse_pairs needs tau, the inlier distance of the consensus")
        kd, pd, rows = self._rows_operand(desc, 0, "desc")
        kx, px, rows_x = self._rows_operand(xyz, 3, "xyz")
        if rows != rows_x:
            raise MvicpError(f"desc has {rows} rows, xyz {rows_x}")
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if len(off) < 2 or int(off[-1]) != rows:
            raise MvicpError("offsets must hold n_sets + 1 values and end at the number of rows")
        src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1); dst = np.ascontiguousarray(dst, dtype=np.int32).reshape(-1)
        E = len(src)
        if len(dst) != E:
            raise MvicpError("src and dst differ in length")
        if seeds is None or isinstance(seeds, (int, np.integer)):
            s0 = 0 if seeds is None else int(seeds)
            sd = np.array([(s0 + e) & (2 ** 64 - 1) for e in range(E)], dtype=np.uint64)
        else:
            sd = np.array([int(v) & (2 ** 64 - 1) for v in seeds], dtype=np.uint64)
            if len(sd) != E:
                raise MvicpError("one seed per edge")
        res = (CoarseEdge * max(E, 1))()
        spare = np.zeros(1, dtype=np.int64)   # (an empty array still gets a pointer that is not NULL)
        ip = lambda a: (a if a.size else spare).ctypes.data_as(C.POINTER(C.c_int))
        got = int(_check(self.lib, self.lib.mvicp_coarse_pairs(self.h, pd, px, off.ctypes.data_as(C.POINTER(C.c_longlong)), len(off) - 1, int(kd.shape[1]), E,
                                                               ip(src), ip(dst), (sd if E else spare).ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                                               int(bool(mutual)), float(ratio), int(hypotheses), float(tau), float(edge_sim), res)))
        assert got == E
        self._coarse_counts = [int(res[e].pairs) for e in range(E)]
        out = {k: np.array([getattr(res[e], k) for e in range(E)], dtype=np.int32) for k in ("pairs", "best", "count", "accepted")}
        out["pose"] = poses_from_c(np.array([res[e].pose[:] for e in range(E)]).reshape(-1, 16)) if E else np.zeros((0, 4, 4))
        return out

    def coarse_pairs_fetch(self, edge, device=False):
        """mvicp_coarse_pairs_fetch: edge `edge` of the last coarse_pairs -> (pairs (c,2) int32 in ascending i, flags (c,) uint8 = the
        winner's inliers).  device=True: torch tensors on the engine's GPU."""
        counts = getattr(self, "_coarse_counts", None)
        c = counts[edge] if counts is not None and 0 <= int(edge) < len(counts) else 0
        mk, ptr, ready, f64, i32, i64, u8 = self._result_arrays(device)
        pairs, flags = mk((c, 2), i32), mk((c,), u8)
        ready()
        _check(self.lib, self.lib.mvicp_coarse_pairs_fetch(self.h, int(edge), c, ptr(pairs), ptr(flags)))
        return pairs, flags

    def nn_query(self, frame, queries, nn_method=NN_AUTO):
        q = np.ascontiguousarray(queries, dtype=np.float64)
        idx = np.zeros(len(q), dtype=np.int32)
        d2 = np.zeros(len(q), dtype=np.float64)
        _check(self.lib, self.lib.mvicp_nn_query(self.h, frame, _dp(q), len(q), nn_method, _ip(idx), _dp(d2)))
        return idx, d2

    # ---- normal equations / S2
    def linearize(self, poses, point_to_plane, robust):
        P = poses_to_c(poses)
        out = np.zeros((self.E, EDGE_BLOCK), dtype=np.float64)
        _check(self.lib, self.lib.mvicp_linearize(self.h, _dp(P), int(point_to_plane), int(robust), _dp(out)))
        return out

    def linearize_pair(self, poses_a, poses_b, point_to_plane, robust):
        """linearize(poses_a), linearize(poses_b) from one pass over the operand stream (bit-identical to the two calls)."""
        Pa, Pb = poses_to_c(poses_a), poses_to_c(poses_b)
        out_a = np.zeros((self.E, EDGE_BLOCK), dtype=np.float64)
        out_b = np.zeros((self.E, EDGE_BLOCK), dtype=np.float64)
        _check(self.lib, self.lib.mvicp_linearize_pair(self.h, _dp(Pa), _dp(Pb), int(point_to_plane), int(robust), _dp(out_a), _dp(out_b)))
        return out_a, out_b

    def linearize_metric(self, poses, metric, robust):
        """linearize with the objective named (METRIC_POINT / METRIC_PLANE / METRIC_SYMMETRIC)."""
        P = poses_to_c(poses)
        out = np.zeros((self.E, EDGE_BLOCK), dtype=np.float64)
        _check(self.lib, self.lib.mvicp_linearize_metric(self.h, _dp(P), int(metric), int(robust), _dp(out)))
        return out

    def optimize_metric(self, poses, fixed, param=PARAM_SOPHUS_SE3, metric=METRIC_SYMMETRIC, robust=True, max_iterations=50):
        """optimize with the objective named; a symmetric solve queues nothing for the next search."""
        b = self._round_buffers(len(poses))
        np.copyto(b["P44"], np.transpose(np.asarray(poses, dtype=np.float64), (0, 2, 1)))
        b["fx"][:] = fixed
        _check(self.lib, self.lib.mvicp_optimize_metric(self.h, b["pP"], b["pfx"], param, int(metric), int(robust), max_iterations, b["psm"]))
        return np.ascontiguousarray(np.transpose(b["P44"], (0, 2, 1))), b["sm"].as_dict()

    def linearize_gicp(self, poses, epsilon=1e-3, robust=True):
        """linearize over the plane-to-plane (Generalized-ICP) objective, C(n) = I - (1 - epsilon) n n^T; epsilon within [1e-6, 1]."""
        P = poses_to_c(poses)
        out = np.zeros((self.E, EDGE_BLOCK), dtype=np.float64)
        _check(self.lib, self.lib.mvicp_linearize_gicp(self.h, _dp(P), float(epsilon), int(robust), _dp(out)))
        return out

    def optimize_gicp(self, poses, fixed, param=PARAM_SOPHUS_SE3, epsilon=1e-3, robust=True, max_iterations=50):
        """optimize over the plane-to-plane objective; like a symmetric solve it queues nothing for the next search."""
        b = self._round_buffers(len(poses))
        np.copyto(b["P44"], np.transpose(np.asarray(poses, dtype=np.float64), (0, 2, 1)))
        b["fx"][:] = fixed
        _check(self.lib, self.lib.mvicp_optimize_gicp(self.h, b["pP"], b["pfx"], param, float(epsilon), int(robust), max_iterations, b["psm"]))
        return np.ascontiguousarray(np.transpose(b["P44"], (0, 2, 1))), b["sm"].as_dict()

    def optimize(self, poses, fixed, param=PARAM_SOPHUS_SE3, point_to_plane=True, robust=True, max_iterations=50):
        b = self._round_buffers(len(poses))
        np.copyto(b["P44"], np.transpose(np.asarray(poses, dtype=np.float64), (0, 2, 1)))
        b["fx"][:] = fixed          # (the solver forces fixed[0] = 1 in this private copy, like icp-ceres.cpp:244,341,417)
        _check(self.lib, self.lib.mvicp_optimize(self.h, b["pP"], b["pfx"], param, int(point_to_plane), int(robust), max_iterations, b["psm"]))
        return np.ascontiguousarray(np.transpose(b["P44"], (0, 2, 1))), b["sm"].as_dict()

    def set_option(self, name, value):
        _check(self.lib, self.lib.mvicp_set_option(self.h, name.encode(), float(value)))

    def nn_census(self):
        out = np.zeros(10)
        _check(self.lib, self.lib.mvicp_nn_census_ex(self.h, _dp(out), 10))
        return {"queries": out[0], "candidates": out[1], "nodes": out[2], "far": out[3], "hits": out[4], "fetched": out[5],
                "rescreens": out[6], "confirm_rounds": out[7], "blocks": out[8], "confirmations": out[9]}

    def last_nn_launch(self):
        """Which NN kernel instantiation the last search launched: "brute", "grid", "tile<WPE,TOP,BND>", "mfma<WPE,TOP,BND,CEN,LBT,ENTRY>"."""
        return self.lib.mvicp_last_nn_launch(self.h).decode()

    # ---- profiling
    def profile(self, on=True):
        """on: False/0 off, True/1 every scope, 2 only the roofline scopes "nn", "linearize" and "linearize_pair"."""
        _check(self.lib, self.lib.mvicp_profile_enable(self.h, int(on)))

    def profile_reset(self):
        _check(self.lib, self.lib.mvicp_profile_reset(self.h))

    def profile_get(self, kernel):
        ms, n, b = C.c_double(), C.c_longlong(), C.c_double()
        _check(self.lib, self.lib.mvicp_profile_get(self.h, kernel.encode(), C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def profile_get_ex(self, kernel):
        """{"ms", "launches", "model_bytes", "survey_bytes", "queries"} of a scope ("nn" = every NN kernel together)."""
        out = np.zeros(5)
        _check(self.lib, self.lib.mvicp_profile_get_ex(self.h, kernel.encode(), _dp(out), 5))
        return {"ms": float(out[0]), "launches": int(out[1]), "model_bytes": float(out[2]), "survey_bytes": float(out[3]), "queries": float(out[4])}

    def sync(self):
        _check(self.lib, self.lib.mvicp_sync(self.h))


def unpack_block(b):
    """91 -> (H 12x12 symmetric, g 12, cost)."""
    H = np.zeros((12, 12))
    iu = np.triu_indices(12)
    H[iu] = b[:78]
    H = H + np.triu(H, 1).T
    return H, np.array(b[78:90]), float(b[90])
