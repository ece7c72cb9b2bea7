"""mvicp_fpfh / mvicp_fpfh_fetch on the MI355X: desc and used equal the numpy statement of the contract (tests/fpfhref.py) byte for byte;
no tolerance anywhere.  What a case must contain (rows cut by max_nn, by the radius, empty rows, ties in the row order, degenerate
pairs, y == 0, swap ties, rows of duplicates only) is asserted on the reference alone, so no case can pass trivially."""
import ctypes as C
import functools

import numpy as np
import pytest

import fpfhref
import knnref
import mvicp
import offorigin as oo
import outlierref
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
# G1: at 3000 points per square metre a radius of 2 / 5 / 8 cm holds about 4 / 24 / 60 points
SHEET_CASES = {2: 0.02, 16: 0.05, 64: 0.08}


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what):
    for key, dt, width in (("desc", np.float64, 33), ("used", np.int32, 1)):
        a = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else got[key]
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(want[key])
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape, (what, key, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            rows = np.unique(bad // width)
            raise AssertionError((what, key, len(bad), len(rows), rows[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), b.reshape(-1)[bad[:4]].tolist()))


@functools.lru_cache(maxsize=None)
def sheet(placement=None):
    """-> (points, normals, sorted rows of the reference)"""
    p, nr, _ = outlierref.sheet_cloud(3000, 7)
    if placement:
        p = oo.place_points(placement, p, shift_extra=oo.WU)
    return p, nr, knnref.sorted_rows(p)


@functools.lru_cache(maxsize=None)
def sheet_ref(max_nn, placement=None):
    p, nr, srt = sheet(placement)
    knn = knnref.from_sorted(*srt, max_nn, SHEET_CASES[max_nn])
    return knn, fpfhref.fpfh(p, nr, SHEET_CASES[max_nn], max_nn, knn)


def check_sheet_case(max_nn, placement=None):
    """Rows cut by max_nn, rows the radius cut short (impossible at max_nn = 2, where a row is the point and one neighbour or the point
    alone) and empty rows."""
    knn, want = sheet_ref(max_nn, placement)
    cnt, m = knn["cnt"], want["used"]
    assert (cnt == max_nn).sum() > 100 and (m == 0).sum() > 20 and (m == cnt - 1).all()
    if max_nn > 2:
        assert ((cnt > 1) & (cnt < max_nn)).sum() > 100
    assert want["degenerate"] == 0 and want["pairs"] > 1000
    return want


# ---- G1
@pytest.mark.parametrize("max_nn", [2, 16, 64])
def test_sheet(eng, max_nn):
    p, nr, _ = sheet()
    want = check_sheet_case(max_nn)
    eng.set_frames([p], [nr])
    assert_same(eng.fpfh(0, SHEET_CASES[max_nn], max_nn), want, ("sheet", max_nn))


# ---- G2
@pytest.mark.parametrize("normals", ["z", "random"])
def test_lattice(eng, normals):
    p = knnref.shuffled_lattice(7, 3)
    nr = fpfhref.z_normals(len(p)) if normals == "z" else fpfhref.unit_normals(len(p), 7)
    srt = knnref.sorted_rows(p)
    eng.set_frames([p], [nr])
    for max_nn, radius in ((12, 1.5), (64, 2.1)):      # 12 cuts the 12 neighbours at d2 = 2 of an interior point after 5: a tie in the row order
        knn = knnref.from_sorted(*srt, max_nn, radius)
        want = fpfhref.fpfh(p, nr, radius, max_nn, knn)
        if max_nn == 12:
            interior = ((p >= 1) & (p <= 5)).all(1)
            assert interior.sum() == 125 and (knn["d2"][interior, 7:12] == 2).all() and (srt[1][interior, 12] == 2).all()
        else:
            assert (knn["cnt"] == 64).sum() == 0 and knn["cnt"].max() == 33 and knn["cnt"].min() == 11   # the radius alone cuts
        if normals == "z":
            assert want["degenerate"] > 0 and want["y_zero"] > 0 and want["swap_ties"] == want["pairs"]
        else:
            assert want["degenerate"] == 0
        assert_same(eng.fpfh(0, radius, max_nn), want, ("lattice", normals, max_nn))


# ---- G3
def test_duplicates(eng):
    p, nr, _ = outlierref.sheet_cloud(1500, 9)
    p = p.copy()
    rng = np.random.Generator(np.random.PCG64(10))
    many = rng.choice(len(p), size=70, replace=False)
    p[many] = p[many[0]]                                 # 70 copies of one point: each of their rows holds 64 entries at d2 == 0 only
    few = rng.choice(np.setdiff1d(np.arange(len(p)), many), size=12, replace=False).reshape(4, 3)
    for trio in few:
        p[trio] = p[trio[0]]                             # four points in three copies each
    radius, max_nn = 0.06, 64
    knn = knnref.knn_search(p, None, max_nn, radius)
    want = fpfhref.fpfh(p, nr, radius, max_nn, knn)
    assert (knn["cnt"][many] == 64).all() and (knn["d2"][many] == 0).all() and (want["used"][many] == 0).all()
    near = np.flatnonzero((knn["idx"] == many.min()).any(1) & (knn["d2"][:, 0] == 0) & (want["used"] > 0))
    assert len(near) > 0                                 # points that have the copies as neighbours: those contribute r_j = 0
    for trio in few:
        assert (knn["d2"][trio, :3] == 0).all() and (knn["d2"][trio, 3] > 0).all() and (want["used"][trio] == knn["cnt"][trio] - 3).all()
    eng.set_frames([p], [nr])
    assert_same(eng.fpfh(0, radius, max_nn), want, "duplicates")


# ---- G4
def test_away_from_the_origin(eng):
    p, nr, _ = sheet("utm")
    assert np.abs(p).max() > 4e6 and np.ptp(p, axis=0).max() < 2.0
    want = check_sheet_case(16, "utm")
    assert not fpfhref.same(want, sheet_ref(16)[1], keys=("desc",))   # the rounding of the coordinates is part of the input
    eng.set_frames([p], [nr])
    assert_same(eng.fpfh(0, SHEET_CASES[16], 16), want, "utm")


# ---- G5
def test_device_destinations_and_the_search_left_behind(eng):
    p, nr, _ = sheet()
    eng.set_frames([p], [nr])
    for max_nn in (16, 64):
        knn, want = sheet_ref(max_nn)
        got = eng.fpfh(0, SHEET_CASES[max_nn], max_nn, device=True)
        assert all(isinstance(got[key], torch.Tensor) and got[key].is_cuda for key in ("desc", "used"))
        assert_same(got, want, ("device", max_nn))
        # the search the call ran is the context's last neighbour-search result
        n = len(p)
        cnt, off = np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
        idx, d2 = np.zeros((n, max_nn), np.int32), np.zeros((n, max_nn))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert eng.lib.mvicp_knn_fetch(eng.h, n, n * max_nn, vp(cnt), vp(off), vp(idx), vp(d2)) == 0
        assert knnref.same({"cnt": cnt, "off": off, "idx": idx, "d2": d2, "total": knn["total"]}, knn)
    # only one of the two destinations
    n = len(p)
    used = np.zeros(n, np.int32)
    assert eng.lib.mvicp_fpfh_fetch(eng.h, n, None, used.ctypes.data_as(C.c_void_p)) == 0 and used.tobytes() == sheet_ref(64)[1]["used"].tobytes()


# ---- G6
def test_errors_and_empty_frames(eng):
    p, nr, _ = sheet()
    small = np.ascontiguousarray(p[:300])
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        desc, used = np.zeros((300, 33)), np.zeros(300, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.mvicp_fpfh_fetch(h, 300, vp(desc), vp(used)) == ERR_STATE and b"mvicp_fpfh first" in lib.mvicp_last_error()   # before any call
        assert lib.mvicp_fpfh(h, 0, 0.05, 16) == ERR_ARG                                                # frames not declared: out of range
        assert lib.mvicp_set_num_frames(h, 4) == 0
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.mvicp_set_frame(h, 0, dp(small), None, 300) == 0                                      # no normals
        assert lib.mvicp_set_frame(h, 1, dp(small), dp(np.ascontiguousarray(nr[:300])), 300) == 0
        empty = np.zeros((0, 3))
        assert lib.mvicp_set_frame(h, 2, dp(empty), dp(empty), 0) == 0
        assert lib.mvicp_fpfh(h, 0, 0.05, 16) == ERR_STATE and b"normals" in lib.mvicp_last_error()
        assert lib.mvicp_fpfh(h, 3, 0.05, 16) == ERR_STATE and b"never uploaded" in lib.mvicp_last_error()
        assert lib.mvicp_fpfh_fetch(h, 300, vp(desc), vp(used)) == ERR_STATE
        assert lib.mvicp_fpfh(h, 1, 0.05, 16) == 300
        assert lib.mvicp_fpfh_fetch(h, 299, vp(desc), None) == ERR_ARG and b"cap_rows" in lib.mvicp_last_error()
        assert lib.mvicp_fpfh_fetch(h, 299, None, vp(used)) == ERR_ARG
        assert lib.mvicp_fpfh_fetch(h, 300, vp(desc), vp(used)) == 0
        want = fpfhref.fpfh(small, nr[:300], 0.05, 16)
        assert (want["used"] > 0).sum() > 100
        assert_same({"desc": desc, "used": used}, want, "300 points")
        # an argument error leaves the last result alone
        for args in ((1, 0.05, 1), (1, 0.05, 65), (1, 0.0, 16), (1, float("nan"), 16), (7, 0.05, 16)):
            assert lib.mvicp_fpfh(h, *args) == ERR_ARG, args
        desc2 = np.zeros((300, 33))
        assert lib.mvicp_fpfh_fetch(h, 300, vp(desc2), None) == 0 and desc2.tobytes() == desc.tobytes()
        # n = 0: zero rows, no error
        assert lib.mvicp_fpfh(h, 2, 0.05, 16) == 0
        assert lib.mvicp_fpfh_fetch(h, 0, None, None) == 0
        got = fresh.fpfh(2, 0.05, 16)
        assert got["desc"].shape == (0, 33) and got["used"].shape == (0,)
        got = fresh.fpfh(2, 0.05, 16, device=True)
        assert tuple(got["desc"].shape) == (0, 33) and tuple(got["used"].shape) == (0,)
        assert lib.mvicp_fpfh(h, 1, 0.05, 16) == 300
        assert lib.mvicp_set_num_frames(h, 1) == 0                                                       # the result ends with the frames
        assert lib.mvicp_fpfh_fetch(h, 1 << 20, None, None) == ERR_STATE
    finally:
        fresh.close()


# ---- G7
def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_fpfh):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_fpfh:
                e.fpfh(2, 0.05, 16)   # before the graph exists
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_fpfh:
                    e.fpfh(r, 0.04, 32)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_fpfh:
                    e.fpfh(3 - r, (0.03, 0.06, 0.02)[r], (64, 2, 33)[r], device=(r == 2))
                triples, offsets = e.map_correspondences()
                epochs = e.correspondence_epochs()
                blocks = e.linearize(poses, True, True)
                poses, sm = e.optimize(poses, pb["fixed"])
                if with_fpfh:
                    e.fpfh(r + 1, 0.05, 16)   # between rounds
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            epochs.tobytes(), sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)
