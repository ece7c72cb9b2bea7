"""-m gpu: mvicp_orient_normals equals its contract (tests/orientref.py) byte for byte -- nrm, flip, comp and the number of components --
on every case of tests/orientcases.py, in all three modes, from the frame's stored normals and from the last estimate, into host and
device destinations; mvicp_orient_adopt leaves what an upload with the same values leaves; every refusal leaves earlier results
fetchable; mvicp_set_num_frames ends the result; non-finite normals, whatever their bits, are an argument error."""
import ctypes as C
import functools

import numpy as np
import pytest

import knnref
import mvicp
import normref
import orientcases as oc
import orientref as oref
from mvicp import synth
from mvicp.lib import METRIC_PLANE, METRIC_SYMMETRIC, ORIENT_ANCHOR, ORIENT_DIRECTION, ORIENT_VIEWPOINT, MvicpError

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def want(name, mode=ORIENT_ANCHOR, ref=None):
    p, N, k, radius = oc.case(name)
    base = want(name) if (mode, ref) != (ORIENT_ANCHOR, None) else None      # (the rows are computed once per case)
    return oref.orient(p, N, k, radius, mode, ref, rows=None if base is None else base["knn"])


def assert_same(got, ref, what):
    assert got["components"] == ref["components"], (what, got["components"], ref["components"])
    for key in ("comp", "flip", "nrm"):
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(ref[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, key, int((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(1).sum()))


@pytest.mark.parametrize("name", oc.CASES)
def test_gpu_equals_the_contract(eng, name):
    p, N, k, radius = oc.case(name)
    ref = want(name)
    eng.set_frames([p], [N])
    assert_same(eng.orient_normals(0, k, radius), ref, name)
    # the search the call ran is the engine's last neighbour-search result
    rows = {"cnt": np.zeros(len(p), dtype=np.int32), "idx": np.zeros((len(p), k), dtype=np.int32)}
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
    assert eng.lib.mvicp_knn_fetch(eng.h, len(p), len(p) * k, ptr(rows["cnt"]), None, ptr(rows["idx"]), None) == 0
    assert rows["cnt"].tobytes() == ref["knn"]["cnt"].tobytes() and rows["idx"].tobytes() == ref["knn"]["idx"].tobytes()
    # the frame's own normals are untouched
    if len(p):
        stored = eng.get_structure(0, "snor").view(np.float64).reshape(-1, 3)[eng.get_structure(0, "inv").view(np.int32)]
        assert stored.tobytes() == N.tobytes()


@pytest.mark.parametrize("name", ["sphere", "islands", "collinear"])
def test_modes(eng, name):
    p, N, k, radius = oc.case(name)
    eng.set_frames([p], [N])
    for mode, ref in ((ORIENT_VIEWPOINT, None), (ORIENT_VIEWPOINT, (0.3, -0.2, 5.0)), (ORIENT_DIRECTION, (0.6, -0.48, 0.64)), (ORIENT_VIEWPOINT, (0.0, 0.0, 0.0))):
        assert_same(eng.orient_normals(0, k, radius, 0, mode, ref), want(name, mode, ref), (name, mode, ref))


def test_votes_a_tie_and_a_component_that_flips(eng):
    p, N = oc.votes()
    eng.set_frames([p], [N])
    anchor = oref.orient(p, N, 4, 0.3)
    assert anchor["components"] == 4 and anchor["comp"].tolist() == [0] * 5 + [5, 6] + [7] * 4
    assert (anchor["nrm"][:5, 0] == 1).all() and (anchor["nrm"][7:, 0] == -1).all()
    assert_same(eng.orient_normals(0, 4, 0.3), anchor, "anchor")
    view = oref.orient(p, N, 4, 0.3, oref.VIEWPOINT, None)
    assert (view["nrm"][:5, 0] == -1).all()                        # A flips: all five look away from the origin
    assert view["nrm"][5, 0] == 1 and view["nrm"][6, 0] == -1     # B: the single points turn towards it
    assert (view["nrm"][7:, 0] == -1).all()                        # C: s = -0.3, -0.1, +0.1, +0.3 times -1: two against two, the sign stays
    assert_same(eng.orient_normals(0, 4, 0.3, 0, ORIENT_VIEWPOINT, None), view, "viewpoint NULL")
    assert_same(eng.orient_normals(0, 4, 0.3, 0, ORIENT_VIEWPOINT, (0.0, 0.0, 0.0)), view, "viewpoint 0")
    tie = oref.orient(p, N, 4, 0.3, oref.VIEWPOINT, (0.0, -9.0, 0.0))
    assert (tie["flip"][7:] == anchor["flip"][7:]).all()
    assert_same(eng.orient_normals(0, 4, 0.3, 0, ORIENT_VIEWPOINT, (0.0, -9.0, 0.0)), tie, "tie")
    along = oref.orient(p, N, 4, 0.3, oref.DIRECTION, (-1.0, 0.0, 0.0))
    assert (along["nrm"][:, 0] == -1).all()
    assert_same(eng.orient_normals(0, 4, 0.3, 0, ORIENT_DIRECTION, (-1.0, 0.0, 0.0)), along, "direction")
    zero = oref.orient(p, N, 4, 0.3, oref.DIRECTION, (0.0, 1.0, 0.0))   # every s is 0: nothing votes
    assert zero["flip"].tobytes() == anchor["flip"].tobytes()
    assert_same(eng.orient_normals(0, 4, 0.3, 0, ORIENT_DIRECTION, (0.0, 1.0, 0.0)), zero, "direction, all zero")


def test_source_1_reads_the_last_estimate_and_device_destinations(eng):
    import torch
    p = oc.case("blob10")[0]
    est = normref.normals(p, 16)
    ref = oref.orient(p, est["nrm"], 10, rows=want("blob10")["knn"])
    eng.set_frames([p, p[:50]], None)
    with pytest.raises(MvicpError):
        eng.orient_normals(0, 10)                                   # source 0: the frame has no normals
    with pytest.raises(MvicpError):
        eng.orient_normals(0, 10, 0.0, 1)                           # source 1: nothing estimated
    got = eng.estimate_normals(0, 16)
    assert got["nrm"].tobytes() == est["nrm"].tobytes()
    with pytest.raises(MvicpError):
        eng.orient_normals(1, 10, 0.0, 1)                           # the estimate is another frame's
    assert_same(eng.orient_normals(0, 10, 0.0, 1), ref, "source 1")
    dev = eng.orient_normals(0, 10, 0.0, 1, device=True)
    assert dev["nrm"].is_cuda and dev["flip"].dtype == torch.uint8 and dev["comp"].dtype == torch.int32
    assert_same({"components": dev["components"], "nrm": dev["nrm"].cpu().numpy(), "flip": dev["flip"].cpu().numpy(), "comp": dev["comp"].cpu().numpy()}, ref, "device")
    # the estimate it read is still there; a mixed fetch: one host, one device destination, one absent
    assert eng.lib.mvicp_normals_fetch(eng.h, len(p), None, None, None) == 0
    flip = torch.empty(len(p), dtype=torch.uint8, device="cuda")
    nrm = np.zeros((len(p), 3))
    assert eng.lib.mvicp_orient_fetch(eng.h, len(p), nrm.ctypes.data_as(C.c_void_p), C.c_void_p(flip.data_ptr()), None) == 0
    assert nrm.tobytes() == ref["nrm"].tobytes() and flip.cpu().numpy().tobytes() == ref["flip"].tobytes()
    assert eng.lib.mvicp_orient_fetch(eng.h, len(p) - 1, nrm.ctypes.data_as(C.c_void_p), None, None) == -1
    eng.set_frame(0, p)                                             # an upload drops the estimate and the orientation
    with pytest.raises(MvicpError):
        eng.orient_normals(0, 10, 0.0, 1)
    assert eng.lib.mvicp_orient_fetch(eng.h, len(p), None, None, None) == -3


def test_every_refusal_leaves_the_earlier_results(eng):
    p, N, k, radius = oc.case("islands")
    ref = want("islands")
    eng.set_frames([p, p[:40], np.zeros((0, 3))], [N, None, None])
    assert eng.lib.mvicp_orient_fetch(eng.h, 1 << 20, None, None, None) == -3
    with pytest.raises(MvicpError):
        eng.adopt_orientation()
    assert_same(eng.orient_normals(0, k, radius), ref, "first")
    search = eng.knn_search(0, None, 5)
    dp = lambda v: np.array(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    call = eng.lib.mvicp_orient_normals
    nan, inf = float("nan"), float("inf")
    table = [((3, 0, 10, 0.0, 0, None), -1), ((-1, 0, 10, 0.0, 0, None), -1), ((0, 2, 10, 0.0, 0, None), -1), ((0, -1, 10, 0.0, 0, None), -1),
             ((0, 0, 1, 0.0, 0, None), -1), ((0, 0, 65, 0.0, 0, None), -1), ((0, 0, 10, 0.0, 3, None), -1), ((0, 0, 10, 0.0, -1, None), -1),
             ((0, 0, 10, nan, 0, None), -1), ((0, 0, 10, inf, 0, None), -1), ((0, 0, 10, 0.0, 2, None), -1), ((0, 0, 10, 0.0, 1, dp([0.0, nan, 0.0])), -1),
             ((0, 0, 10, 0.0, 2, dp([inf, 0.0, 0.0])), -1), ((1, 0, 10, 0.0, 0, None), -3), ((0, 1, 10, 0.0, 0, None), -3)]
    for args, status in table:
        assert call(eng.h, *args) == status, args
        out = {"components": ref["components"], "nrm": np.zeros_like(ref["nrm"]), "flip": np.zeros_like(ref["flip"]), "comp": np.zeros_like(ref["comp"])}
        assert eng.lib.mvicp_orient_fetch(eng.h, len(p), *(out[key].ctypes.data_as(C.c_void_p) for key in ("nrm", "flip", "comp"))) == 0
        assert_same(out, ref, args)
        again = np.zeros((len(p), 5), dtype=np.int32)
        assert eng.lib.mvicp_knn_fetch(eng.h, len(p), len(p) * 5, None, None, again.ctypes.data_as(C.c_void_p), None) == 0
        assert again.tobytes() == search["idx"].tobytes()
    got = eng.orient_normals(2, 10)                                  # an empty frame: no rows, no components, not an error
    assert got["components"] == 0 and got["nrm"].shape == (0, 3) and got["flip"].shape == (0,)
    assert eng.lib.mvicp_orient_fetch(eng.h, 0, None, None, None) == 0
    # a non-finite normal is reported by the call and leaves no result behind
    inside = int(np.flatnonzero(np.bincount(ref["comp"], minlength=len(p))[ref["comp"]] > 1)[0])   # a point with neighbours
    bad = N.copy(); bad[inside, 1] = np.inf
    eng.set_frame(0, p, bad)
    assert call(eng.h, 0, 0, k, radius, 0, None) == -1
    assert eng.lib.mvicp_orient_fetch(eng.h, 1 << 20, None, None, None) == -3


def test_set_num_frames_ends_the_result(eng):
    p, N, k, radius = oc.case("islands")
    eng.set_frames([p], [N])
    assert_same(eng.orient_normals(0, k, radius), want("islands"), "islands")
    assert eng.lib.mvicp_orient_fetch(eng.h, len(p), None, None, None) == 0
    assert eng.lib.mvicp_set_num_frames(eng.h, 1) == 0              # the same count: the frames are new ones all the same
    assert eng.lib.mvicp_orient_fetch(eng.h, 1 << 20, None, None, None) == -3
    assert eng.lib.mvicp_orient_adopt(eng.h) == -3
    # and the stage works again afterwards, on buffers of its own again
    eng.set_frames([p], [N])
    assert_same(eng.orient_normals(0, k, radius), want("islands"), "islands, again")


def test_non_finite_normals_of_unequal_payloads_are_an_argument_error(eng):
    """NaNs of different payloads and signs: the two ends of an edge may see different bits for its dot, whatever the hook graph then
    looks like the call reports the normals (MVICP_ERR_ARG), not an internal limit."""
    p, N, k, radius = oc.case("blob10")
    bits = np.array([0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000123, 0xfff4000000000000, 0x7ff0000000000000, 0xfff0000000000000], dtype=np.uint64)
    bad = N.copy()
    rng = np.random.default_rng(5)
    rows = rng.choice(len(p), len(p) // 2, replace=False)
    bad[rows, rng.integers(0, 3, len(rows))] = bits.view(np.float64)[rng.integers(0, len(bits), len(rows))]
    eng.set_frames([p], [bad])
    assert eng.lib.mvicp_orient_normals(eng.h, 0, 0, k, radius, 0, None) == -1
    assert eng.lib.mvicp_orient_fetch(eng.h, 1 << 20, None, None, None) == -3
    eng.set_frame(0, p, N)
    assert_same(eng.orient_normals(0, k, radius), want("blob10"), "blob10 after the refusal")


K_EST, VIEW = 16, (0.0, 0.0, 2.0)


@functools.lru_cache(maxsize=None)
def world():
    """-> (problem of three clouds of 1500 points, per cloud the contract's normals, oriented by the contract)"""
    pb = synth.make_problem(3, 1500)
    nrm = [oref.orient(p, normref.normals(p, K_EST, 0.0, VIEW)["nrm"], 10, 0.0, oref.DIRECTION, (0.0, 0.0, -1.0))["nrm"] for p in pb["pts"]]
    return pb, nrm


def blocks(e, pb):
    return tuple(np.asarray(e.linearize_metric(pb["init"], m, True)).tobytes() for m in (METRIC_PLANE, METRIC_SYMMETRIC))


@pytest.mark.parametrize("case", ["before the first search", "between a search and a solve", "a frame uploaded without normals"])
def test_adopted_orientation_is_what_an_upload_of_the_values_leaves(case):
    pb, nrm = world()
    twin = mvicp.Engine(0)
    e = mvicp.Engine(0)
    try:
        twin.set_frames(pb["pts"], nrm); twin.set_graph(pb["src"], pb["dst"])
        twin.correspond(pb["init"], pb["fixed"], 0.05)
        twin_blocks = blocks(twin, pb)

        def adopt_all():
            for i in range(3):
                e.estimate_normals(i, K_EST, 0.0, VIEW)
                got = e.orient_normals(i, 10, 0.0, 1, ORIENT_DIRECTION, (0.0, 0.0, -1.0))
                assert got["nrm"].tobytes() == nrm[i].tobytes()
                e.adopt_orientation()
                out = np.zeros_like(nrm[i])   # (the result stays fetchable after adoption)
                assert e.lib.mvicp_orient_fetch(e.h, len(out), out.ctypes.data_as(C.c_void_p), None, None) == 0 and out.tobytes() == nrm[i].tobytes()

        e.set_frames(pb["pts"], None if case.startswith("a frame") else pb["nor"])
        if case == "before the first search":
            adopt_all()
            e.set_graph(pb["src"], pb["dst"])
            e.correspond(pb["init"], pb["fixed"], 0.05)
        else:
            e.set_graph(pb["src"], pb["dst"])
            e.correspond(pb["init"], pb["fixed"], 0.05)
            if case.startswith("a frame"):
                with pytest.raises(MvicpError):
                    e.linearize_metric(pb["init"], METRIC_PLANE, True)
            else:
                assert blocks(e, pb) != twin_blocks
            adopt_all()
        assert blocks(e, pb) == twin_blocks
        for i in range(3):
            assert e.get_structure(i, "snor").view(np.float64).reshape(-1, 3)[e.get_structure(i, "inv").view(np.int32)].tobytes() == nrm[i].tobytes()
        e.correspond(pb["init"], pb["fixed"], 0.05)
        assert blocks(e, pb) == twin_blocks
        # mvicp_normals_adopt still adopts the estimate, not the orientation
        est = e.estimate_normals(0, K_EST, 0.0, VIEW)
        e.adopt_normals()
        assert e.get_structure(0, "snor").view(np.float64).reshape(-1, 3)[e.get_structure(0, "inv").view(np.int32)].tobytes() == est["nrm"].tobytes()
    finally:
        e.close(); twin.close()
