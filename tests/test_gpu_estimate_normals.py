"""mvicp_estimate_normals / mvicp_normals_fetch on the MI355X: nrm, curvature and used equal the numpy statement of the contract
(tests/normref.py) byte for byte, signs of zeros included; no tolerance anywhere.  What a case must contain (exact ties, rows of
duplicates, short rows, rows the radius cut below 3, flipped normals, negative zeros, s == 0) is asserted on the reference alone, so no
case can pass trivially.  Then the behaviour of the call: the search it leaves behind, history neutrality, refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import knnref
import mvicp
import normcases
import normref
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what):
    for key, dt, width in (("nrm", np.float64, 3), ("curvature", np.float64, 1), ("used", np.int32, 1)):
        a = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else got[key]
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(want[key])
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape, (what, key, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            rows = np.unique(bad // width)
            raise AssertionError((what, key, len(bad), len(rows), rows[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), b.reshape(-1)[bad[:4]].tolist()))


@functools.lru_cache(maxsize=None)
def blob():
    """-> (700 points, sorted rows of the reference)"""
    p = np.ascontiguousarray(np.random.default_rng(31).normal(0.0, 0.25, (700, 3)))
    return p, knnref.sorted_rows(p)


@functools.lru_cache(maxsize=None)
def blob_ref(k, radius=0.0, vp=None):
    p, srt = blob()
    return normref.normals(p, k, radius, vp, knnref.from_sorted(*srt, k, radius))


VIEW = (0.3, -0.2, 0.1)   # inside the blob: normals are flipped on every side of it


@pytest.mark.parametrize("k", [3, 10, 64])
def test_blob(eng, k):
    p, _ = blob()
    want = blob_ref(k, 0.0, VIEW)
    c = want["curvature"]
    assert (want["used"] == k).all() and ((c > 0).sum() > 300 and (c == 0).sum() > 100 if k == 3 else (c > 0).all())   # three points span a plane
    eng.set_frames([p], None)
    assert_same(eng.estimate_normals(0, k, 0.0, VIEW), want, ("blob", k))


def test_quantised_lattice_with_exact_ties(eng):
    p = normcases.placed("lattice", 1.0, 0.0, 700)
    srt = knnref.sorted_rows(p)
    assert (srt[1][:, 9] == srt[1][:, 10]).sum() > 50 and (srt[1][:, 15] == srt[1][:, 16]).sum() > 50   # ties at the cut of both k
    eng.set_frames([p], None)
    for k in (10, 16):
        want = normref.normals(p, k, 0.0, (0.5, 0.5, 3.0), knnref.from_sorted(*srt, k, 0.0))
        assert_same(eng.estimate_normals(0, k, 0.0, (0.5, 0.5, 3.0)), want, ("lattice", k))


def test_duplicates_and_collinear(eng):
    dup, line = normcases.duplicates(), normcases.collinear()
    eng.set_frames([dup, line], None)
    want = normref.normals(dup, 10, 0.0, (0.0, 0.0, 1.0))
    assert (dup[want["knn"]["idx"]] == dup[:, None, :]).all() and (want["curvature"] == 0).all()   # C = 0: no rotation, V = I
    assert_same(eng.estimate_normals(0, 10, 0.0, (0.0, 0.0, 1.0)), want, "duplicates, rows of copies only")
    want = normref.normals(dup, 40, 0.0, (0.0, 0.0, 1.0))
    assert (want["curvature"] > 0).sum() > 50 and (want["curvature"] == 0).sum() > 50   # two sites: rank one, l lands on either side of 0
    assert_same(eng.estimate_normals(0, 40, 0.0, (0.0, 0.0, 1.0)), want, "duplicates, the copies of two sites")
    want = normref.normals(line, 10, 0.0, (0.0, 0.0, 10.0))
    assert np.isfinite(want["nrm"]).all()
    assert_same(eng.estimate_normals(1, 10, 0.0, (0.0, 0.0, 10.0)), want, "collinear")


def test_small_scale_away_from_the_origin(eng):
    p = normcases.placed("blob", 1e-3, 1e3, 700)
    assert np.abs(p).min(0).max() > 0.4 and np.ptp(p, axis=0).max() < 3e-3
    eng.set_frames([p], None)
    for vp in (None, tuple(p.mean(0))):
        want = normref.normals(p, 16, 0.0, vp)
        assert_same(eng.estimate_normals(0, 16, 0.0, vp), want, ("scale 1e-3 offset 1e3", vp))


def test_hybrid_rows_short_and_full(eng):
    p, _ = blob()
    want = blob_ref(12, 0.11, VIEW)
    u = want["used"]
    assert (u < 3).sum() > 20 and (u == 12).sum() > 50 and ((u >= 3) & (u < 12)).sum() > 50
    assert not want["nrm"][u < 3].any() and not np.signbit(want["nrm"][u < 3]).any()
    eng.set_frames([p], None)
    assert_same(eng.estimate_normals(0, 12, 0.11, VIEW), want, "hybrid")


def test_rows_shorter_than_the_tree_and_tiny_clouds(eng):
    rng = np.random.default_rng(4)
    p40, p2, p0 = rng.normal(0, 0.2, (40, 3)), rng.normal(0, 0.2, (2, 3)), np.zeros((0, 3))
    eng.set_frames([p40, p2, p0], None)
    want = normref.normals(p40, 64, 0.0, VIEW)
    assert (want["used"] == 40).all()
    assert_same(eng.estimate_normals(0, 64, 0.0, VIEW), want, "n = 40 at max_nn = 64")
    want = normref.normals(p2, 5, 0.0, VIEW)
    assert (want["used"] == 2).all() and not want["nrm"].any()
    assert_same(eng.estimate_normals(1, 5, 0.0, VIEW), want, "n = 2")
    got = eng.estimate_normals(2, 5, 0.0, VIEW)
    assert got["nrm"].shape == (0, 3) and got["curvature"].shape == (0,) and got["used"].shape == (0,)
    got = eng.estimate_normals(2, 5, 0.0, VIEW, device=True)
    assert tuple(got["nrm"].shape) == (0, 3)
    assert eng.lib.mvicp_normals_fetch(eng.h, 0, None, None, None) == 0


def test_viewpoints_null_zero_own_position_and_a_flipped_half(eng):
    p, _ = blob()
    eng.set_frames([p], None)
    want = blob_ref(10)
    a, b = eng.estimate_normals(0, 10, 0.0, None), eng.estimate_normals(0, 10, 0.0, (0.0, 0.0, 0.0))
    assert_same(a, want, "NULL viewpoint"); assert_same(b, want, "explicit zeros")
    # the viewpoint at point 5's own position: w = 0, s == 0 keeps n, whatever side it points to
    vp = tuple(p[5])
    want = blob_ref(10, 0.0, vp)
    raw = blob_ref(10, 0.0, tuple(p[5] + want["nrm"][5]))   # (seen from the side n points to: certainly not flipped)
    assert want["nrm"][5].tobytes() == raw["nrm"][5].tobytes()
    assert_same(eng.estimate_normals(0, 10, 0.0, vp), want, "viewpoint at a point")
    # two exact planes z = 0 and z = 1 seen from between them: (+0, +0, +1) below, (-0, -0, -1) above
    rng = np.random.default_rng(9)
    xy = rng.uniform(0, 1, (600, 2))
    planes = np.ascontiguousarray(np.column_stack([xy, np.repeat([0.0, 1.0], 300)]))
    want = normref.normals(planes, 8, 0.0, (0.5, 0.5, 0.5))
    up, down = want["nrm"][:300], want["nrm"][300:]
    assert (up == [0, 0, 1]).all() and not np.signbit(up).any()
    assert (down == [0, 0, -1]).all() and np.signbit(down).all()
    eng.set_frames([planes], None)
    assert_same(eng.estimate_normals(0, 8, 0.0, (0.5, 0.5, 0.5)), want, "flipped half")


def test_device_destinations_device_upload_and_the_search_left_behind(eng):
    p, srt = blob()
    dev = torch.device("cuda", 0)
    eng.set_frames([p[:10]], None)
    eng.set_frame_device(0, torch.from_numpy(p).to(dev))
    for k, radius in ((10, 0.0), (64, 0.2)):
        knn = knnref.from_sorted(*srt, k, radius)
        want = normref.normals(p, k, radius, VIEW, knn)
        got = eng.estimate_normals(0, k, radius, VIEW, device=True)
        assert all(isinstance(got[key], torch.Tensor) and got[key].is_cuda for key in ("nrm", "curvature", "used"))
        assert_same(got, want, ("device", k))
        # the search the call ran is the context's last neighbour-search result
        n = len(p)
        cnt, off = np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
        idx, d2 = np.zeros((n, k), np.int32), np.zeros((n, k))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert eng.lib.mvicp_knn_fetch(eng.h, n, n * k, vp(cnt), vp(off), vp(idx), vp(d2)) == 0
        assert knnref.same({"cnt": cnt, "off": off, "idx": idx, "d2": d2, "total": knn["total"]}, knn)
        assert knnref.same(eng.knn_search(0, None, k, radius), knn)
    # only one of the destinations
    curv = np.zeros(len(p))
    assert eng.lib.mvicp_normals_fetch(eng.h, len(p), None, curv.ctypes.data_as(C.c_void_p), None) == 0
    assert curv.tobytes() == want["curvature"].tobytes()


def test_history_neutral():
    pb = synth.make_problem(2, 3000)

    def run(with_est):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_est:
                e.estimate_normals(1, 16)   # before the graph exists
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_est:
                    e.estimate_normals(r % 2, 30, 0.0, (0.0, 0.0, 1.0))
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_est:
                    e.estimate_normals(1 - r % 2, (64, 3, 33)[r], (0.03, 0.0, 0.06)[r], device=(r == 2))
                triples, offsets = e.map_correspondences()
                epochs = e.correspondence_epochs()
                blocks = e.linearize(poses, True, True)
                poses, sm = e.optimize(poses, pb["fixed"])
                if with_est:
                    e.estimate_normals(0, 16)   # between rounds
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            epochs.tobytes(), sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_refusals_leave_the_earlier_result_and_the_context():
    p, _ = blob()
    small = np.ascontiguousarray(p[:300])
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        nrm, curv, used = np.zeros((300, 3)), np.zeros(300), np.zeros(300, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        view = np.array(VIEW)
        assert lib.mvicp_normals_fetch(h, 300, vp(nrm), vp(curv), vp(used)) == ERR_STATE and b"mvicp_estimate_normals first" in lib.mvicp_last_error()
        assert lib.mvicp_normals_adopt(h) == ERR_STATE
        assert lib.mvicp_estimate_normals(None, 0, 10, 0.0, None) == ERR_ARG
        assert lib.mvicp_normals_fetch(None, 0, None, None, None) == ERR_ARG and lib.mvicp_normals_adopt(None) == ERR_ARG
        assert lib.mvicp_estimate_normals(h, 0, 10, 0.0, None) == ERR_ARG                              # frames not declared: out of range
        assert lib.mvicp_set_num_frames(h, 3) == 0
        assert lib.mvicp_set_frame(h, 0, dp(small), None, 300) == 0
        assert lib.mvicp_set_frame(h, 1, dp(p), None, len(p)) == 0
        fresh.n_frames, fresh.npts = 3, [300, len(p), 0]                                              # (what Engine.set_frames keeps)
        assert lib.mvicp_estimate_normals(h, 2, 10, 0.0, None) == ERR_STATE and b"never uploaded" in lib.mvicp_last_error()
        assert lib.mvicp_normals_fetch(h, 300, vp(nrm), None, None) == ERR_STATE
        assert lib.mvicp_estimate_normals(h, 0, 10, 0.0, dp(view)) == 300
        knn0 = fresh.knn_search(0, None, 10, 0.0)                                                     # (replaces the search result; same rows)
        assert lib.mvicp_estimate_normals(h, 0, 10, 0.0, dp(view)) == 300
        assert lib.mvicp_normals_fetch(h, 299, vp(nrm), None, None) == ERR_ARG and b"cap_rows" in lib.mvicp_last_error()
        assert lib.mvicp_normals_fetch(h, 300, vp(nrm), vp(curv), vp(used)) == 0
        want = normref.normals(small, 10, 0.0, VIEW)
        assert_same({"nrm": nrm, "curvature": curv, "used": used}, want, "300 points")
        # every refusal leaves the last result, the last search and the frame alone
        bad_view = [np.array(v) for v in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf))]
        refusals = [(0, 2, 0.0, None), (0, 65, 0.0, None), (0, 10, float("nan"), None), (0, 10, float("inf"), None), (-1, 10, 0.0, None),
                    (3, 10, 0.0, None)] + [(0, 10, 0.0, dp(v)) for v in bad_view]
        for args in refusals:
            assert lib.mvicp_estimate_normals(h, *args) == ERR_ARG, args[:3]
        assert lib.mvicp_estimate_normals(h, 2, 10, 0.0, None) == ERR_STATE
        nrm2, curv2, used2 = np.zeros((300, 3)), np.zeros(300), np.zeros(300, np.int32)
        assert lib.mvicp_normals_fetch(h, 300, vp(nrm2), vp(curv2), vp(used2)) == 0
        assert nrm2.tobytes() == nrm.tobytes() and curv2.tobytes() == curv.tobytes() and used2.tobytes() == used.tobytes()
        n = 300
        cnt, idx = np.zeros(n, np.int32), np.zeros((n, 10), np.int32)
        assert lib.mvicp_knn_fetch(h, n, n * 10, vp(cnt), None, vp(idx), None) == 0
        assert cnt.tobytes() == knn0["cnt"].tobytes() and idx.tobytes() == knn0["idx"].tobytes()
        # the estimate does not touch the frame: it still has no normals, and a plane evaluation keeps refusing it
        assert fresh.get_structure(0, "snor").size == 0
        # the result ends with an upload to ITS frame, not with one to another frame
        assert lib.mvicp_set_frame(h, 1, dp(small), None, 300) == 0
        assert lib.mvicp_normals_fetch(h, 300, vp(nrm2), None, None) == 0
        assert lib.mvicp_set_frame(h, 0, dp(small), None, 300) == 0
        assert lib.mvicp_normals_fetch(h, 300, vp(nrm2), None, None) == ERR_STATE
        assert lib.mvicp_estimate_normals(h, 0, 10, 0.0, dp(view)) == 300
        assert lib.mvicp_set_num_frames(h, 1) == 0                                                     # the result ends with the frames
        assert lib.mvicp_normals_fetch(h, 1 << 20, None, None, None) == ERR_STATE
    finally:
        fresh.close()
