"""ctypes binding of mv-lm-icp_amd/bin/frame_harness.so (tests/frame_harness.cpp): the Frame / Session / ICP_Ceres mirror of
host/frame.h driven from Python.  Test infrastructure only.  One `Mirror` per process: the session behind it is process-wide."""
import ctypes as C
import os

import numpy as np

import mvicp
from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_PATH = os.environ.get("MVICP_FRAME_HARNESS") or os.path.join(ROOT, "mv-lm-icp_amd", "bin", "frame_harness.so")   # the variable: comparison builds only

SYMBOLS = [
    "fh_last_error", "fh_reset_all", "fh_slot_create", "fh_slot_destroy", "fh_slot_recreate", "fh_slot_address", "fh_vec_set", "fh_vec_destroy",
    "fh_set_pts", "fh_set_nor", "fh_stash_set", "fh_stash_swap_pts", "fh_get_pts", "fh_get_nor", "fh_set_pose", "fh_get_pose", "fh_set_fixed", "fh_get_fixed", "fh_get_version",
    "fh_set_neighbours", "fh_num_neighbours", "fh_get_edge", "fh_set_option", "fh_counters", "fh_invalidate", "fh_invalidate_lists",
    "fh_session_reset", "fh_pose_knn", "fh_closest_to_neighbours", "fh_ceres", "fh_optimize", "fh_get_closest_point", "fh_get_closest_points",
    "fh_get_neighbours", "fh_get_neighbour_indices", "fh_recompute_normals", "fh_voxel_downsample", "fh_remove_outliers", "fh_iss_keypoints",
    "fh_fused_model", "fh_result_cloud", "fh_result_indices", "fh_overlap_neighbours", "fh_init_from_features",
]

FRESH, IN_PLACE = 0, 1                                  # how fh_set_pts / fh_set_nor store a cloud
OPT_COPY_BACK, OPT_COPY_THREADS, OPT_NN_METHOD = 0, 1, 2
CERES_QUATERNION, CERES_ANGLE_AXIS, CERES_SOPHUS = 0, 1, 2
CORR_DTYPE = mvicp.Engine.CORR_DTYPE


class MirrorError(RuntimeError):
    """An exception the mirror threw, with its text."""


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    mvicp.load_library()   # (the harness links the library; loaded first so that both share one instance)
    if not os.path.exists(HARNESS_PATH):
        raise MirrorError(f"{HARNESS_PATH} not found: build it with `make -C mv-lm-icp_amd` (or __graft_entry__.build())")
    lib = C.CDLL(HARNESS_PATH)
    vp, ip, dp, fp, llp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_longlong)
    ullp = C.POINTER(C.c_ulonglong)
    lib.fh_last_error.restype = C.c_char_p
    lib.fh_reset_all.argtypes = []
    lib.fh_slot_create.argtypes = [ip]
    lib.fh_slot_destroy.argtypes = [C.c_int]
    lib.fh_slot_recreate.argtypes = [C.c_int]
    lib.fh_slot_address.argtypes = [C.c_int, ullp]
    lib.fh_vec_set.argtypes = [C.c_int, ip, C.c_int]
    lib.fh_vec_destroy.argtypes = [C.c_int]
    lib.fh_set_pts.argtypes = [C.c_int, dp, C.c_int, C.c_int]
    lib.fh_set_nor.argtypes = [C.c_int, dp, C.c_int, C.c_int]
    lib.fh_stash_set.argtypes = [dp, C.c_int]
    lib.fh_stash_swap_pts.argtypes = [C.c_int]
    lib.fh_get_pts.argtypes = [C.c_int, dp, C.c_longlong, llp]
    lib.fh_get_nor.argtypes = [C.c_int, dp, C.c_longlong, llp]
    lib.fh_set_pose.argtypes = [C.c_int, dp]
    lib.fh_get_pose.argtypes = [C.c_int, dp]
    lib.fh_set_fixed.argtypes = [C.c_int, C.c_int]
    lib.fh_get_fixed.argtypes = [C.c_int, ip]
    lib.fh_get_version.argtypes = [C.c_int, ullp]
    lib.fh_set_neighbours.argtypes = [C.c_int, ip, fp, C.c_int]
    lib.fh_num_neighbours.argtypes = [C.c_int, ip]
    lib.fh_get_edge.argtypes = [C.c_int, C.c_int, ip, fp, llp, vp, C.c_longlong]
    lib.fh_set_option.argtypes = [C.c_int, C.c_int]
    lib.fh_counters.argtypes = [ullp, ullp]
    lib.fh_invalidate.argtypes = []
    lib.fh_invalidate_lists.argtypes = []
    lib.fh_session_reset.argtypes = []
    lib.fh_pose_knn.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.fh_closest_to_neighbours.argtypes = [C.c_int, C.c_int, C.c_float]
    lib.fh_ceres.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.fh_optimize.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(L.Summary)]
    lib.fh_get_closest_point.argtypes = [C.c_int, dp, llp, dp]
    lib.fh_get_closest_points.argtypes = [C.c_int, dp, C.c_int, llp, dp]
    lib.fh_get_neighbours.argtypes = [C.c_int, C.c_int, C.c_int, dp]
    lib.fh_get_neighbour_indices.argtypes = [C.c_int, C.c_int, ip, C.c_longlong]
    lib.fh_recompute_normals.argtypes = [C.c_int]
    lib.fh_voxel_downsample.argtypes = [C.c_int, C.c_double, llp, llp]
    lib.fh_remove_outliers.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, llp, llp]
    lib.fh_iss_keypoints.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, llp]
    lib.fh_fused_model.argtypes = [C.c_int, C.c_double, llp, llp]
    lib.fh_result_cloud.argtypes = [dp, dp]
    lib.fh_result_indices.argtypes = [ip]
    lib.fh_overlap_neighbours.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.c_double, ip]
    lib.fh_init_from_features.argtypes = [C.c_int, dp, ip, ip]
    _lib = lib
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


class Mirror:
    """The harness's calls with numpy arguments.  Frames are addressed by SLOT (their storage); a vector of frames (0 or 1) lists slots, and
    the calls the reference makes with a position in the vector take that position."""

    def __init__(self):
        self.lib = load()

    def _ck(self, st):
        if st != 0:
            raise MirrorError(self.lib.fh_last_error().decode())

    # ---- frames and vectors
    def reset_all(self):
        self._ck(self.lib.fh_reset_all())

    def slot_create(self):
        s = C.c_int(-1)
        self._ck(self.lib.fh_slot_create(C.byref(s)))
        return s.value

    def slot_destroy(self, s):
        self._ck(self.lib.fh_slot_destroy(s))

    def slot_recreate(self, s):
        self._ck(self.lib.fh_slot_recreate(s))

    def slot_address(self, s):
        a = C.c_ulonglong(0)
        self._ck(self.lib.fh_slot_address(s, C.byref(a)))
        return a.value

    def vec_set(self, v, slots):
        a = np.ascontiguousarray(list(slots) + [0], dtype=np.int32)
        self._ck(self.lib.fh_vec_set(v, _ip(a), len(a) - 1))

    def vec_destroy(self, v):
        self._ck(self.lib.fh_vec_destroy(v))

    # ---- members
    def set_pts(self, s, xyz, mode=FRESH):
        a = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self._ck(self.lib.fh_set_pts(s, _dp(a) if len(a) else None, len(a), mode))

    def set_nor(self, s, xyz, mode=FRESH):
        a = np.zeros((0, 3)) if xyz is None else np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self._ck(self.lib.fh_set_nor(s, _dp(a) if len(a) else None, len(a), mode))

    def stash_set(self, xyz):
        """the harness's spare vector <- a fresh vector holding xyz"""
        a = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        self._ck(self.lib.fh_stash_set(_dp(a) if len(a) else None, len(a)))

    def stash_swap_pts(self, s):
        """std::vector::swap between the frame's `pts` and the spare vector: buffers change hands, nothing is copied"""
        self._ck(self.lib.fh_stash_swap_pts(s))

    def _cloud(self, fn, s):
        n = C.c_longlong(0)
        self._ck(fn(s, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3))
        self._ck(fn(s, _dp(out) if n.value else None, n.value, C.byref(n)))
        return out

    def get_pts(self, s):
        return self._cloud(self.lib.fh_get_pts, s)

    def get_nor(self, s):
        return self._cloud(self.lib.fh_get_nor, s)

    def set_pose(self, s, pose):
        self._ck(self.lib.fh_set_pose(s, _dp(L.poses_to_c(np.asarray(pose, dtype=np.float64).reshape(1, 4, 4)))))

    def get_pose(self, s):
        out = np.zeros(16)
        self._ck(self.lib.fh_get_pose(s, _dp(out)))
        return L.poses_from_c(out)[0]

    def set_fixed(self, s, fixed):
        self._ck(self.lib.fh_set_fixed(s, int(bool(fixed))))

    def get_fixed(self, s):
        f = C.c_int(0)
        self._ck(self.lib.fh_get_fixed(s, C.byref(f)))
        return bool(f.value)

    def get_version(self, s):
        v = C.c_ulonglong(0)
        self._ck(self.lib.fh_get_version(s, C.byref(v)))
        return v.value

    def set_neighbours(self, s, idx, weights=None):
        a = np.ascontiguousarray(list(idx) + [0], dtype=np.int32)
        w = np.zeros(len(a), dtype=np.float32)
        if weights is not None:
            w[:len(a) - 1] = weights
        self._ck(self.lib.fh_set_neighbours(s, _ip(a), w.ctypes.data_as(C.POINTER(C.c_float)), len(a) - 1))

    def num_neighbours(self, s):
        n = C.c_int(0)
        self._ck(self.lib.fh_num_neighbours(s, C.byref(n)))
        return n.value

    def get_edge(self, s, j):
        """-> (neighbour, weight as np.float32, the list as a CORR_DTYPE array)"""
        nb, w, n = C.c_int(0), C.c_float(0), C.c_longlong(0)
        self._ck(self.lib.fh_get_edge(s, j, C.byref(nb), C.byref(w), C.byref(n), None, 0))
        out = np.zeros(n.value, dtype=CORR_DTYPE)
        self._ck(self.lib.fh_get_edge(s, j, C.byref(nb), C.byref(w), C.byref(n), out.ctypes.data_as(C.c_void_p) if n.value else None, n.value))
        return nb.value, np.float32(w.value), out

    def get_edges(self, s):
        return [self.get_edge(s, j) for j in range(self.num_neighbours(s))]

    # ---- session
    def set_option(self, which, value):
        self._ck(self.lib.fh_set_option(which, int(value)))

    def counters(self):
        c, s = C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.lib.fh_counters(C.byref(c), C.byref(s)))
        return c.value, s.value

    def invalidate(self):
        self._ck(self.lib.fh_invalidate())

    def invalidate_lists(self):
        self._ck(self.lib.fh_invalidate_lists())

    def session_reset(self):
        self._ck(self.lib.fh_session_reset())

    # ---- the reference's calls
    def pose_knn(self, v, i, k):
        self._ck(self.lib.fh_pose_knn(v, i, k))

    def closest_to_neighbours(self, v, i, thresh):
        self._ck(self.lib.fh_closest_to_neighbours(v, i, np.float32(thresh)))

    def ceres(self, v, which=CERES_SOPHUS, point_to_plane=True, robust=True):
        self._ck(self.lib.fh_ceres(v, which, int(point_to_plane), int(robust)))

    def optimize(self, v, param, metric, robust=True):
        sm = L.Summary()
        self._ck(self.lib.fh_optimize(v, param, metric, int(robust), C.byref(sm)))
        return sm.as_dict()

    def get_closest_point(self, s, q):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(3)
        i, d = C.c_longlong(-1), C.c_double(0)
        self._ck(self.lib.fh_get_closest_point(s, _dp(q), C.byref(i), C.byref(d)))
        return i.value, d.value

    def get_closest_points(self, s, q):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
        idx = np.zeros(len(q) + 1, dtype=np.int64); d2 = np.zeros(len(q) + 1)
        self._ck(self.lib.fh_get_closest_points(s, _dp(q) if len(q) else None, len(q), idx.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(d2)))
        return idx[:-1], d2[:-1]

    def get_neighbours(self, s, query, k):
        out = np.zeros((max(k, 1), 3))
        self._ck(self.lib.fh_get_neighbours(s, query, k, _dp(out)))
        return out[:k]

    def get_neighbour_indices(self, s, k, n):
        out = np.zeros((n, max(k, 1)), dtype=np.int32)
        self._ck(self.lib.fh_get_neighbour_indices(s, k, _ip(out), out.size))
        return out[:, :k] if k >= 1 else out

    def recompute_normals(self, s):
        self._ck(self.lib.fh_recompute_normals(s))

    def _result_cloud(self, n_pts, n_nor):
        pts = np.zeros((n_pts, 3)); nor = np.zeros((n_nor, 3))
        self._ck(self.lib.fh_result_cloud(_dp(pts) if n_pts else None, _dp(nor) if n_nor else None))
        return pts, (nor if n_nor else None)

    def voxel_downsample(self, s, voxel):
        a, b = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.fh_voxel_downsample(s, voxel, C.byref(a), C.byref(b)))
        return self._result_cloud(a.value, b.value)

    def remove_outliers(self, s, k, std_ratio, radius):
        a, b = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.fh_remove_outliers(s, k, std_ratio, radius, C.byref(a), C.byref(b)))
        return self._result_cloud(a.value, b.value)

    def iss_keypoints(self, s, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5):
        n = C.c_longlong(0)
        self._ck(self.lib.fh_iss_keypoints(s, salient_radius, non_max_radius, gamma21, gamma32, min_neighbors, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        self._ck(self.lib.fh_result_indices(_ip(out) if n.value else None))
        return out

    def fused_model(self, v, voxel):
        a, b = C.c_longlong(0), C.c_longlong(0)
        self._ck(self.lib.fh_fused_model(v, voxel, C.byref(a), C.byref(b)))
        return self._result_cloud(a.value, b.value)

    def overlap_neighbours(self, v, knn, thresh, max_samples=4096, min_fraction=0.0):
        c = C.c_int(0)
        self._ck(self.lib.fh_overlap_neighbours(v, knn, np.float32(thresh), max_samples, min_fraction, C.byref(c)))
        return c.value

    def init_from_features(self, v, voxel=0.0, radius=0.0, tau=0.0, edge_sim=0.9, max_nn=64, min_count=3, hypotheses=10000, seed=0, refine=True,
                           keypoints=0, salient_radius=0.0, nms_radius=0.0, gamma21=0.975, gamma32=0.975, min_neighbors=5):
        o = np.array([voxel, radius, tau, edge_sim, max_nn, min_count, hypotheses, seed, float(bool(refine)), keypoints, salient_radius, nms_radius,
                      gamma21, gamma32, min_neighbors], dtype=np.float64)
        c, e = C.c_int(0), C.c_int(0)
        self._ck(self.lib.fh_init_from_features(v, _dp(o), C.byref(c), C.byref(e)))
        return c.value, e.value
