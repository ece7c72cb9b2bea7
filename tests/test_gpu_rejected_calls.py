"""-m gpu: a call that is REFUSED changes nothing a caller can see.

The set-up calls (mvicp_set_num_frames, mvicp_set_frame, mvicp_set_frame_device, mvicp_set_shard, mvicp_set_graph, mvicp_set_correspondences,
mvicp_recompute_normals, mvicp_set_option) and the argument / call-order errors of mvicp_linearize, mvicp_linearize_pair, mvicp_optimize,
mvicp_nn_query, mvicp_get_correspondences, mvicp_map_correspondences and mvicp_correspondence_epochs are held to one rule (include/mvicp.h
states it per entry): a non-OK return leaves the context as it was.  (mvicp_correspond's own guard is tests/test_gpu_search_state.py's.)

One twin harness, the shape of the stages' test_history_neutral: a script runs on context A with the refused calls in it and on context B
without them, in lockstep, and after every step everything observable is compared as bytes -- before a graph exists every structure of
mvicp_get_structure of the touched frame and one batch of 64 mvicp_nn_query answers; from each of three rounds counts, weights, the triples
and offsets of mvicp_map_correspondences, epochs, the blocks of mvicp_linearize, the poses of mvicp_optimize and its iterations and final
cost.  Every refused call also asserts its status and a fragment of mvicp_last_error().  A refused call may change the error string,
profile counters and performance-only state (queued evaluations, cache validity): nothing of that is compared.

Two post-conditions were defects and are spelled out:
  uploads  mvicp_set_frame / mvicp_set_frame_device found a non-finite coordinate only AFTER the old cloud, its structures and its tie tree
           were released and the new bytes were on the device: the frame was left with n > 0, NaN points, no structures and no build error,
           and a later search or query ran a silent brute force over those bytes.  Now the frame is exactly what it was -- a held cloud
           (test_refused_calls_change_nothing) or empty (test_refused_uploads_onto_an_empty_frame_leave_it_empty).
  normals  mvicp_recompute_normals allocated the normal buffers of a frame uploaded without normals before it looked at k: a refused call
           (k = 2, 17, 0, -1) left two uninitialised buffers, and point-to-plane evaluation -- which takes a non-null buffer for "has
           normals" -- was no longer refused.  Now it still returns MVICP_ERR_STATE naming that frame.

Problem: synth.make_problem(3, 800); variants: every frame with normals, none, and only frame 1 without (the error then names frame 1)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
OK, ARG, HIP, STATE = 0, -1, -2, -3
CUTOFF = 0.05
END = object()


@pytest.fixture(scope="module")
def pb():
    return synth.make_problem(3, 800)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


class Side:
    """One of the twins: `rejects` says whether the refused calls of the script are made on it."""

    def __init__(self, rejects):
        self.E = mvicp.Engine(0)
        self.rejects = rejects
        self.poses = None

    def status(self, name, *args):
        lib = self.E.lib
        st = int(getattr(lib, name)(self.E.h, *args))
        return st, lib.mvicp_last_error().decode()

    def reject(self, status, fragment, name, *args):
        if not self.rejects:
            return
        st, msg = self.status(name, *args)
        assert st == status and fragment in msg, (name, "expected", status, fragment, "got", st, msg)


def canon(v):
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, v.tobytes())
    if isinstance(v, (tuple, list)):
        return tuple(canon(x) for x in v)
    if isinstance(v, float):
        return np.float64(v).tobytes()
    return v


def describe(a, b):
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        if a.shape != b.shape or a.dtype != b.dtype:
            return "shapes %s %s / %s %s" % (a.dtype, a.shape, b.dtype, b.shape)
        return "%d of %d bytes differ" % (int((np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8)).sum()), a.nbytes)
    return "%r / %r" % (a, b)


def twin(script):
    """script(side) is a generator of (tag, value): A (with the refused calls) and B (without) advance in lockstep."""
    A, B = Side(True), Side(False)
    seen = 0
    try:
        ga, gb = script(A), script(B)
        while True:
            a, b = next(ga, END), next(gb, END)
            assert (a is END) == (b is END), "the twins' scripts have different lengths"
            if a is END:
                break
            assert a[0] == b[0], (a[0], b[0])
            assert canon(a[1]) == canon(b[1]), ("differs from the twin that made no refused call", a[0], describe(a[1], b[1]))
            seen += 1
    finally:
        A.E.close(); B.E.close()
    return seen


# ---------------------------------------------------------------- what is observed
def structures(X, frame):
    for name in L.STRUCTURE_NAMES:
        yield ("structure", frame, name), X.E.get_structure(frame, name)


def queries(X, frame, q):
    idx, d2 = X.E.nn_query(frame, q)
    yield ("nn_query", frame), (idx, d2)


def frame_state(X, frame, q):
    yield from structures(X, frame)
    yield from queries(X, frame, q)


def empty_frame_state(X, frame, q):
    yield ("structure of an empty frame", frame), X.status("mvicp_get_structure", frame, b"spts", None, 0)
    idx = np.zeros(len(q), dtype=np.int32); d2 = np.zeros(len(q))
    yield ("nn_query of an empty frame", frame), X.status("mvicp_nn_query", frame, L._dp(q), len(q), L.NN_AUTO, L._ip(idx), L._dp(d2))


def round_(X, tag, fixed, plane, robust, param, sym=False):
    E = X.E
    c, w = E.correspond(X.poses, fixed, CUTOFF)
    yield (tag, "counts"), c
    yield (tag, "weights"), w
    t, o = E.map_correspondences()
    yield (tag, "offsets"), o
    yield (tag, "triples"), t
    yield (tag, "epochs"), E.correspondence_epochs()
    yield (tag, "blocks"), E.linearize(X.poses, plane, robust)
    P, sm = E.optimize(X.poses, fixed, param, plane, bool(robust), 50)
    yield (tag, "poses"), P
    yield (tag, "iterations, final cost"), (int(sm["iterations"]), float(sm["final_cost"]))
    if sym:   # (every frame has normals) the symmetric objective on the same lists, from the same poses; its result is observed, not adopted
        yield (tag, "symmetric blocks"), E.linearize_metric(X.poses, L.METRIC_SYMMETRIC, robust)
        Ps, sms = E.optimize_metric(X.poses, fixed, param, L.METRIC_SYMMETRIC, bool(robust), 50)
        yield (tag, "symmetric poses"), Ps
        yield (tag, "symmetric iterations, final cost"), (int(sms["iterations"]), float(sms["final_cost"]))
    X.poses = P


# ---------------------------------------------------------------- the refused calls
def bad_clouds(good):
    out = {}
    for name, row, col, val in (("NaN in the first row", 0, 0, np.nan), ("+Inf in the first row", 0, 2, np.inf),
                                ("NaN in the last row", len(good) - 1, 1, np.nan), ("+Inf in the last row", len(good) - 1, 2, np.inf)):
        bad = good.copy()
        bad[row, col] = val
        out[name] = bad
    return out


def refused_uploads(X, frame, good, n_frames, with_graph):
    """every refused mvicp_set_frame / mvicp_set_frame_device onto `frame`; a generator of nothing (so that a script can interleave
    observations: `for _ in refused_uploads(...): yield from observe`)"""
    nrm = np.ascontiguousarray(good[:, ::-1])
    dgood, dnrm = _dev(good), _dev(nrm)
    torch.cuda.synchronize()
    for entry, xyz, nor in (("mvicp_set_frame", L._dp(good), L._dp(nrm)), ("mvicp_set_frame_device", dgood.data_ptr(), dnrm.data_ptr())):
        if with_graph:
            X.reject(STATE, "set frames before mvicp_set_graph", entry, frame, xyz, nor, len(good))
            yield entry
            continue
        X.reject(ARG, "out of range", entry, n_frames, xyz, nor, len(good)); yield entry
        X.reject(ARG, "out of range", entry, -1, xyz, nor, len(good)); yield entry
        X.reject(ARG, "bad cloud", entry, frame, xyz, nor, -1); yield entry
        X.reject(ARG, "bad cloud", entry, frame, None, nor, 5); yield entry
    if with_graph:
        return
    for name, bad in bad_clouds(good).items():
        X.reject(ARG, "non-finite coordinate in cloud", "mvicp_set_frame", frame, L._dp(bad), L._dp(nrm), len(bad)); yield name
        X.reject(ARG, "non-finite coordinate in cloud", "mvicp_set_frame", frame, L._dp(bad), None, len(bad)); yield name
        dbad = _dev(bad)
        torch.cuda.synchronize()
        X.reject(ARG, "non-finite coordinate in cloud", "mvicp_set_frame_device", frame, dbad.data_ptr(), dnrm.data_ptr(), len(bad)); yield name
        X.reject(ARG, "non-finite coordinate in cloud", "mvicp_set_frame_device", frame, dbad.data_ptr(), None, len(bad)); yield name
    # a host pointer handed to the device path
    X.reject(ARG, "xyz is not", "mvicp_set_frame_device", frame, good.ctypes.data, None, len(good)); yield "host pointer"
    X.reject(ARG, "nrm is not", "mvicp_set_frame_device", frame, dgood.data_ptr(), nrm.ctypes.data, len(good)); yield "host pointer"


def refused_graphs(X, n_frames):
    ok = np.array([1, 2], dtype=np.int32)
    X.reject(ARG, "bad edge list", "mvicp_set_graph", 2, None, L._ip(ok))
    X.reject(ARG, "bad edge list", "mvicp_set_graph", 2, L._ip(ok), None)
    X.reject(ARG, "bad edge list", "mvicp_set_graph", -1, L._ip(ok), L._ip(ok))
    src, dst = np.array([1, 2], dtype=np.int32), np.array([0, n_frames], dtype=np.int32)
    X.reject(ARG, "invalid", "mvicp_set_graph", 2, L._ip(src), L._ip(dst))
    src, dst = np.array([1, -1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    X.reject(ARG, "invalid", "mvicp_set_graph", 2, L._ip(src), L._ip(dst))
    src, dst = np.array([1, 2], dtype=np.int32), np.array([0, 2], dtype=np.int32)   # a self edge
    X.reject(ARG, "invalid", "mvicp_set_graph", 2, L._ip(src), L._ip(dst))


def refused_normals(X, npts, first_only=False, frames=None):
    """every refused mvicp_recompute_normals, on every frame (with normals or without); first_only: only k = 2, 17, 0"""
    K = len(npts)
    for frame in (range(K) if frames is None else frames):
        n = npts[frame]
        nrm = np.zeros((n, 3)); knn = np.zeros((n, 17), dtype=np.int32)
        for k in (2, 17, 0):
            X.reject(ARG, "outside [3, 16]", "mvicp_recompute_normals", frame, k, L._dp(nrm), None)
        if first_only:
            continue
        X.reject(ARG, "outside [3, 16]", "mvicp_recompute_normals", frame, -1, L._dp(nrm), L._ip(knn))
        X.reject(ARG, "outside [3, 16]", "mvicp_recompute_normals", frame, -1, None, None)
        X.reject(STATE, "points < k", "mvicp_recompute_normals", frame, n + 1, L._dp(nrm), None)
    if first_only:
        return
    X.reject(ARG, "out of range", "mvicp_recompute_normals", K, 10, None, None)
    X.reject(ARG, "out of range", "mvicp_recompute_normals", -1, 10, None, None)


def refused_options_and_shards(X, with_graph):
    X.reject(ARG, "unknown option", "mvicp_set_option", b"no_such_option", 1.0)
    X.reject(ARG, "null option name", "mvicp_set_option", None, 1.0)
    X.reject(ARG, "match_chunk must be", "mvicp_set_option", b"match_chunk", 0.0)
    X.reject(ARG, "nn_search_factor", "mvicp_set_option", b"nn_search_factor", -1.0)
    X.reject(ARG, "grid_target out of range", "mvicp_set_option", b"grid_target", 0.0)
    X.reject(ARG, "bad shard", "mvicp_set_shard", 0, 0)
    X.reject(ARG, "bad shard", "mvicp_set_shard", 1, 1)
    X.reject(ARG, "bad shard", "mvicp_set_shard", -1, 2)
    if with_graph:
        X.reject(STATE, "before mvicp_set_graph", "mvicp_set_shard", 0, 1)
        X.reject(STATE, "before mvicp_set_graph", "mvicp_set_shard", 1, 2)
    X.reject(ARG, "n_frames < 0", "mvicp_set_num_frames", -1)


def refused_queries(X, q, n_frames):
    idx = np.zeros(len(q), dtype=np.int32); d2 = np.zeros(len(q))
    X.reject(ARG, "out of range", "mvicp_nn_query", n_frames, L._dp(q), len(q), L.NN_AUTO, L._ip(idx), L._dp(d2))
    X.reject(ARG, "out of range", "mvicp_nn_query", -1, L._dp(q), len(q), L.NN_AUTO, L._ip(idx), L._dp(d2))
    X.reject(ARG, "bad query buffers", "mvicp_nn_query", 0, None, len(q), L.NN_AUTO, L._ip(idx), L._dp(d2))
    X.reject(ARG, "bad query buffers", "mvicp_nn_query", 0, L._dp(q), len(q), L.NN_AUTO, None, L._dp(d2))
    X.reject(ARG, "bad query buffers", "mvicp_nn_query", 0, L._dp(q), len(q), L.NN_AUTO, L._ip(idx), None)
    X.reject(ARG, "bad query buffers", "mvicp_nn_query", 0, L._dp(q), -1, L.NN_AUTO, L._ip(idx), L._dp(d2))
    X.reject(ARG, "unknown nn_method 99", "mvicp_nn_query", 0, L._dp(q), len(q), 99, L._ip(idx), L._dp(d2))
    X.reject(ARG, "unknown nn_method -1", "mvicp_nn_query", 0, L._dp(q), len(q), -1, L._ip(idx), L._dp(d2))


def refused_evaluations(X, poses, fixed, E_edges, have_lists, plane_refused_frame):
    """mvicp_linearize / _pair / mvicp_optimize / the list getters.  E_edges == 0: no graph yet; have_lists False: a graph, no list yet;
    plane_refused_frame: the frame a point-to-plane evaluation must name (None: every target has normals)."""
    P = L.poses_to_c(poses)
    out = np.zeros((max(E_edges, 1), L.EDGE_BLOCK)); out2 = out.copy()
    fx = np.ascontiguousarray(fixed, dtype=np.uint8).copy()
    sm = L.Summary()
    first = np.zeros(4096, dtype=np.int32); second = first.copy(); dist = np.zeros(4096)
    tp, op, ep = C.c_void_p(), C.POINTER(C.c_longlong)(), C.POINTER(C.c_ulonglong)()
    X.reject(ARG, "null argument", "mvicp_linearize", None, 0, 0, L._dp(out))
    X.reject(ARG, "null argument", "mvicp_linearize_pair", L._dp(P), None, 0, 0, L._dp(out), L._dp(out2))
    # the entry points that name the objective: a metric outside mvicp_metric is refused before anything else is looked at
    for metric in (3, -1):
        X.reject(ARG, "metric %d is not an mvicp_metric" % metric, "mvicp_linearize_metric", L._dp(P), metric, 1, L._dp(out))
        X.reject(ARG, "metric %d is not an mvicp_metric" % metric, "mvicp_optimize_metric", L._dp(P), _u8(fx), 2, metric, 1, 50, C.byref(sm))
    X.reject(ARG, "null argument", "mvicp_linearize_metric", None, L.METRIC_SYMMETRIC, 1, L._dp(out))
    X.reject(ARG, "null argument", "mvicp_linearize_metric", L._dp(P), L.METRIC_SYMMETRIC, 1, None)
    if E_edges == 0:
        X.reject(STATE, "no graph", "mvicp_linearize_metric", L._dp(P), L.METRIC_SYMMETRIC, 1, L._dp(out))
        X.reject(STATE, "no graph", "mvicp_optimize_metric", L._dp(P), _u8(fx), 2, L.METRIC_SYMMETRIC, 1, 50, C.byref(sm))
        X.reject(STATE, "no graph", "mvicp_linearize", L._dp(P), 0, 0, L._dp(out))
        X.reject(STATE, "no graph", "mvicp_linearize_pair", L._dp(P), L._dp(P), 0, 0, L._dp(out), L._dp(out2))
        X.reject(STATE, "no graph", "mvicp_optimize", L._dp(P), _u8(fx), 2, 0, 0, 50, C.byref(sm))
        X.reject(ARG, "out of range", "mvicp_get_correspondences", 0, 4096, L._ip(first), L._ip(second), L._dp(dist))
        X.reject(STATE, "no correspondences yet", "mvicp_map_correspondences", C.byref(tp), C.byref(op))
        X.reject(STATE, "no graph", "mvicp_correspondence_epochs", C.byref(ep))
        X.reject(ARG, "out of range", "mvicp_set_correspondences", 0, 1, L._ip(first), L._ip(second), np.float32(0.01))
        return
    for param in (3, -1):
        X.reject(ARG, "unknown parameterization", "mvicp_optimize", L._dp(P), _u8(fx), param, 0, 1, 50, C.byref(sm))
        X.reject(ARG, "unknown parameterization", "mvicp_optimize_metric", L._dp(P), _u8(fx), param, L.METRIC_SYMMETRIC, 1, 50, C.byref(sm))
    X.reject(ARG, "out of range", "mvicp_get_correspondences", E_edges, 4096, L._ip(first), L._ip(second), L._dp(dist))
    X.reject(ARG, "out of range", "mvicp_get_correspondences", -1, 4096, L._ip(first), L._ip(second), L._dp(dist))
    X.reject(ARG, "null output", "mvicp_map_correspondences", None, C.byref(op))
    if not have_lists:
        X.reject(STATE, "no correspondences", "mvicp_linearize", L._dp(P), 0, 0, L._dp(out))
        X.reject(STATE, "no correspondences", "mvicp_linearize_pair", L._dp(P), L._dp(P), 0, 0, L._dp(out), L._dp(out2))
        X.reject(STATE, "no correspondences", "mvicp_optimize", L._dp(P), _u8(fx), 2, 0, 0, 50, C.byref(sm))
        X.reject(STATE, "no correspondences", "mvicp_linearize_metric", L._dp(P), L.METRIC_SYMMETRIC, 1, L._dp(out))
        X.reject(STATE, "no correspondences", "mvicp_optimize_metric", L._dp(P), _u8(fx), 2, L.METRIC_SYMMETRIC, 1, 50, C.byref(sm))
        X.reject(STATE, "no correspondences yet", "mvicp_get_correspondences", 0, 4096, L._ip(first), L._ip(second), L._dp(dist))
        X.reject(STATE, "no correspondences yet", "mvicp_map_correspondences", C.byref(tp), C.byref(op))
        return
    X.reject(ARG, "capacity", "mvicp_get_correspondences", 1, 1, L._ip(first), L._ip(second), L._dp(dist))
    if plane_refused_frame is not None:
        needs = "point-to-plane needs normals on frame %d" % plane_refused_frame
        X.reject(STATE, needs, "mvicp_linearize", L._dp(P), 1, 1, L._dp(out))
        X.reject(STATE, needs, "mvicp_linearize_pair", L._dp(P), L._dp(P), 1, 0, L._dp(out), L._dp(out2))
        X.reject(STATE, needs, "mvicp_optimize", L._dp(P), _u8(fx), 2, 1, 1, 50, C.byref(sm))
        X.reject(STATE, needs, "mvicp_linearize_metric", L._dp(P), L.METRIC_PLANE, 1, L._dp(out))
        X.reject(STATE, needs, "mvicp_optimize_metric", L._dp(P), _u8(fx), 2, L.METRIC_PLANE, 1, 50, C.byref(sm))
        assert np.array_equal(P, L.poses_to_c(poses))   # (a refused solve returns the caller's poses)


def refused_lists(X, edge, n_src, n_dst, E_edges):
    ok_f = np.arange(8, dtype=np.int32); ok_s = np.arange(8, dtype=np.int32)
    big = np.zeros(n_src + 1, dtype=np.int32)
    X.reject(ARG, "out of range", "mvicp_set_correspondences", E_edges, 8, L._ip(ok_f), L._ip(ok_s), np.float32(0.01))
    X.reject(ARG, "out of range", "mvicp_set_correspondences", -1, 8, L._ip(ok_f), L._ip(ok_s), np.float32(0.01))
    X.reject(ARG, "exceeds the edge capacity", "mvicp_set_correspondences", edge, n_src + 1, L._ip(big), L._ip(big), np.float32(0.01))
    X.reject(ARG, "exceeds the edge capacity", "mvicp_set_correspondences", edge, -1, L._ip(ok_f), L._ip(ok_s), np.float32(0.01))
    for which, val in (("first", n_src), ("first", -1), ("second", n_dst), ("second", -1)):   # an index out of range in the LAST entry
        f, s = ok_f.copy(), ok_s.copy()
        (f if which == "first" else s)[-1] = val
        X.reject(ARG, "correspondence 7 out of range", "mvicp_set_correspondences", edge, 8, L._ip(f), L._ip(s), np.float32(0.01))
    X.reject(ARG, "null correspondence list", "mvicp_set_correspondences", edge, 8, None, L._ip(ok_s), np.float32(0.01))
    X.reject(ARG, "null correspondence list", "mvicp_set_correspondences", edge, 8, L._ip(ok_f), None, np.float32(0.01))


def upload_all(E, pts, nor, path):
    if path == "host":
        E.set_frames(pts, nor)
    else:
        E.set_frames_device([_dev(p) for p in pts], [None if n is None else _dev(n) for n in nor])


def normals_of(pb, variant):
    return [None if (variant == "none" or (variant == "mixed" and k == 1)) else pb["nor"][k] for k in range(len(pb["pts"]))]


# ---------------------------------------------------------------- the scripts
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("variant", ["all", "none", "mixed"])
def test_refused_calls_change_nothing(pb, variant, path):
    pts, src, dst, fixed = pb["pts"], pb["src"], pb["dst"], pb["fixed"]
    nor = normals_of(pb, variant)
    K, E_edges = len(pts), len(src)
    npts = [len(p) for p in pts]
    plane = 1 if variant == "all" else 0
    sym = variant == "all"     # the symmetric observables need normals on both ends of every non-empty list
    q = np.ascontiguousarray(pts[1][:64] + 0.003)
    other = np.ascontiguousarray(pts[2][:500])   # what the refused uploads carry: another cloud, of another size

    def script(X):
        E = X.E
        X.poses = np.array(pb["init"]).copy()
        refused_options_and_shards(X, False)
        upload_all(E, pts, nor, path)
        yield from frame_state(X, 1, q)
        # -- no graph yet: refused uploads onto frame 1, which holds a cloud (the post-condition "uploads")
        for _ in refused_uploads(X, 1, other, K, False):
            yield from frame_state(X, 1, q)
        refused_graphs(X, K)
        refused_normals(X, npts)
        refused_options_and_shards(X, False)
        refused_queries(X, q, K)
        refused_evaluations(X, X.poses, fixed, 0, False, None)
        for k in range(K):
            yield from frame_state(X, k, q)
        E.set_graph(src, dst)
        # -- a graph, no list yet
        for _ in refused_uploads(X, 1, other, K, True):
            pass
        refused_graphs(X, K)
        refused_normals(X, npts)
        refused_options_and_shards(X, True)
        refused_evaluations(X, X.poses, fixed, E_edges, False, None)
        refused_lists(X, 0, npts[src[0]], npts[dst[0]], E_edges)
        refused_evaluations(X, X.poses, fixed, E_edges, False, None)   # (a refused list is no list)
        yield from round_(X, "round 1", fixed, plane, 1, L.PARAM_SOPHUS_SE3, sym)
        # -- a graph with searched lists: the old graph and its lists must keep working
        counts = E.counts
        named = next((int(dst[e]) for e in range(E_edges) if counts[e] > 0 and nor[dst[e]] is None), None)
        assert (named is None) == (variant == "all") and (variant != "mixed" or named == 1), (variant, named, counts)
        refused_normals(X, npts, first_only=True)
        # the post-condition "normals": point-to-plane is still refused, naming the frame without normals
        refused_evaluations(X, X.poses, fixed, E_edges, True, named)
        refused_graphs(X, K)
        refused_normals(X, npts)
        refused_evaluations(X, X.poses, fixed, E_edges, True, named)
        for _ in refused_uploads(X, 1, other, K, True):
            pass
        refused_lists(X, 1, npts[src[1]], npts[dst[1]], E_edges)
        refused_queries(X, q, K)
        refused_options_and_shards(X, True)
        yield ("lists after the refused calls", "epochs"), E.correspondence_epochs()
        for e in range(E_edges):
            yield ("lists after the refused calls", e), E.get_correspondences(e)
        yield ("blocks after the refused calls",), E.linearize(X.poses, plane, 1)
        yield from round_(X, "round 2", fixed, plane, 1, L.PARAM_ANGLE_AXIS, sym)
        refused_graphs(X, K)
        refused_normals(X, npts)
        refused_lists(X, 2, npts[src[2]], npts[dst[2]], E_edges)
        refused_evaluations(X, X.poses, fixed, E_edges, True, named)
        yield from round_(X, "round 3", fixed, plane, 0, L.PARAM_EIGEN_QUATERNION, sym)
        # -- an explicit list survives the refused attempts to replace it
        f0, s0, _ = E.get_correspondences(0)
        E.set_correspondences(0, f0[:50], s0[:50], 0.01)
        refused_lists(X, 0, npts[src[0]], npts[dst[0]], E_edges)
        refused_normals(X, npts)
        yield ("explicit list", "epochs"), E.correspondence_epochs()
        yield ("explicit list", "list"), E.get_correspondences(0)
        yield ("explicit list", "blocks"), E.linearize(X.poses, plane, 1)
        P, sm = E.optimize(X.poses, fixed, L.PARAM_SOPHUS_SE3, plane, True, 50)
        yield ("explicit list", "poses"), P
        yield ("explicit list", "iterations, final cost"), (int(sm["iterations"]), float(sm["final_cost"]))
        if sym:
            yield ("explicit list", "symmetric blocks"), E.linearize_metric(X.poses, L.METRIC_SYMMETRIC, 1)
        # a recompute that is NOT refused still works afterwards, on frames with normals and without
        for k in range(K):
            yield ("recompute_normals", k), E.recompute_normals(k, 10, want_knn=True)
        yield ("blocks with recomputed normals",), E.linearize(P, 1, 1)
        yield ("symmetric blocks with recomputed normals",), E.linearize_metric(P, L.METRIC_SYMMETRIC, 1)    # (every frame has normals now)

    assert twin(script) > 200


@pytest.mark.parametrize("path", ["host", "device"])
def test_refused_uploads_onto_an_empty_frame_leave_it_empty(pb, path):
    """Frame 1 is EMPTY when the non-finite clouds arrive: it stays empty -- mvicp_get_structure and mvicp_nn_query report the empty
    frame, and a graph and a registration through it equal the twin's."""
    pts = [pb["pts"][0], np.zeros((0, 3)), pb["pts"][2]]
    nor = [pb["nor"][0], np.zeros((0, 3)), pb["nor"][2]]
    src, dst, fixed = pb["src"], pb["dst"], pb["fixed"]
    q = np.ascontiguousarray(pb["pts"][1][:64] + 0.003)
    other = np.ascontiguousarray(pb["pts"][1])

    def script(X):
        E = X.E
        X.poses = np.array(pb["init"]).copy()
        upload_all(E, pts, nor, path)
        yield from empty_frame_state(X, 1, q)
        for _ in refused_uploads(X, 1, other, 3, False):
            yield from empty_frame_state(X, 1, q)
        if X.rejects:
            st, msg = X.status("mvicp_get_structure", 1, b"spts", None, 0)
            assert st == STATE and "has no structures (n = 0)" in msg, (st, msg)
            idx = np.zeros(len(q), dtype=np.int32); d2 = np.zeros(len(q))
            st, msg = X.status("mvicp_nn_query", 1, L._dp(q), len(q), L.NN_AUTO, L._ip(idx), L._dp(d2))
            assert st == STATE and "frame 1 is empty" in msg, (st, msg)
        for k in (0, 2):
            yield from frame_state(X, k, q)
        E.set_graph(src, dst)
        for r in range(3):
            yield from round_(X, "round %d" % (r + 1), fixed, 1, 1, L.PARAM_SOPHUS_SE3)
            if r == 0:
                assert all(E.counts[e] == 0 for e in range(len(src)) if src[e] == 1 or dst[e] == 1), E.counts
                assert E.counts.sum() > 0, E.counts
            refused_normals(X, [len(p) for p in pts], frames=(0, 2))

    assert twin(script) > 100


def test_refused_normals_on_a_source_without_normals_keep_symmetric_refused(pb):
    """The symmetric objective reads the SOURCE frame's normals too.  Frame 2 is only ever a source (graph 2 -> 0, 1 -> 0) and was uploaded without
    normals: a refused mvicp_recompute_normals on it (k = 2, 17) must not leave it looking as if it had normals — SYMMETRIC still returns
    MVICP_ERR_STATE naming frame 2, linearize and solve — while POINT and PLANE (whose targets have normals) give the twin's bytes.  A
    recompute that is not refused then makes the symmetric evaluation work, with the twin's bytes."""
    pts, nor = pb["pts"], [pb["nor"][0], pb["nor"][1], None]
    src, dst, fixed = [2, 1], [0, 0], pb["fixed"]
    npts = [len(p) for p in pts]
    needs = "symmetric needs normals on frame 2"

    def refused_symmetric(X):
        P = L.poses_to_c(X.poses)
        out = np.zeros((2, L.EDGE_BLOCK)); fx = np.ascontiguousarray(fixed, dtype=np.uint8).copy(); sm = L.Summary()
        X.reject(STATE, needs, "mvicp_linearize_metric", L._dp(P), L.METRIC_SYMMETRIC, 1, L._dp(out))
        X.reject(STATE, needs, "mvicp_optimize_metric", L._dp(P), _u8(fx), 2, L.METRIC_SYMMETRIC, 1, 50, C.byref(sm))
        assert np.array_equal(P, L.poses_to_c(X.poses)) and not np.any(out)

    def script(X):
        E = X.E
        X.poses = np.array(pb["init"]).copy()
        E.set_frames(pts, nor); E.set_graph(src, dst)
        c, w = E.correspond(X.poses, fixed, CUTOFF)
        assert c[0] > 0, c
        yield ("counts",), c
        refused_symmetric(X)
        refused_normals(X, npts, first_only=True, frames=(2,))
        refused_symmetric(X)
        for metric in (L.METRIC_POINT, L.METRIC_PLANE):
            yield ("blocks", metric), E.linearize_metric(X.poses, metric, 1)
        yield ("epochs",), E.correspondence_epochs()
        for e in range(2):
            yield ("list", e), E.get_correspondences(e)
        P, sm = E.optimize_metric(X.poses, fixed, L.PARAM_SOPHUS_SE3, L.METRIC_POINT, True, 50)
        yield ("point poses",), P
        yield ("point iterations, final cost",), (int(sm["iterations"]), float(sm["final_cost"]))
        refused_symmetric(X)
        yield ("recompute_normals", 2), E.recompute_normals(2, 10)
        yield ("symmetric blocks",), E.linearize_metric(X.poses, L.METRIC_SYMMETRIC, 1)
        Ps, sms = E.optimize_metric(X.poses, fixed, L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
        yield ("symmetric poses",), Ps
        yield ("symmetric iterations, final cost",), (int(sms["iterations"]), float(sms["final_cost"]))

    assert twin(script) == 12
