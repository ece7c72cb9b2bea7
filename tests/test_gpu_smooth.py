"""mvicp_smooth_points / mvicp_smooth_fetch on the MI355X: xyz, shift, moved, H, K and the four outputs of mvicp_fit_normals equal the numpy
statement of the contract (tests/smoothref.py) byte for byte, signs of zeros included; no tolerance anywhere.  What a case must contain is
asserted on the reference alone.  Then the slots: the normals of the call are mvicp_fit_normals' for every call that reads that slot, a
later fit drops the smoothing result, and a refused call leaves it fetchable."""
import ctypes as C

import numpy as np
import pytest

import jetcases
import jetref
import mvicp
import normcases
import smoothref
from test_gpu_fit_normals import assert_same, KEYS as FIT_KEYS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
CASES = jetcases.exact_cases()
KEYS = FIT_KEYS + (("xyz", np.float64, 3), ("shift", np.float64, 1), ("moved", np.uint8, 1), ("H", np.float64, 1), ("K", np.float64, 1))
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blob_ref():
    """the reference of blob-16-3 without a limit, computed once"""
    p, k, r, vp, degree = CASES["blob-16-3"]
    return smoothref.smooth(p, k, r, vp, degree, 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_reference(eng, name):
    p, k, r, vp, degree = CASES[name]
    want = smoothref.smooth(p, k, r, vp, degree, 0.0)
    fitted, moved = want["fitted"].astype(bool), want["moved"].astype(bool)
    assert (moved == fitted).all() and len(p) <= 343
    if name.startswith("blob"):
        assert fitted.all() and want["H"].all() and want["K"].all() and want["shift"].all()
    elif name.startswith("lattice"):
        assert (~fitted).sum() >= 6 and fitted.sum() >= 100      # failed pivots next to fits
    elif name.startswith("hybrid"):
        assert (want["used"] < jetref.TERMS[degree]).sum() > 50 and fitted.sum() > 50
    else:
        assert not fitted.any() and want["xyz"].tobytes() == p.tobytes()      # duplicates: h == 0; collinear: a zero pivot
    eng.set_frames([p], None)
    assert_same(eng.smooth_points(0, k, r, vp, degree), want, name, KEYS)


def test_small_scale_away_from_the_origin(eng):
    p = normcases.placed("blob", 1e-3, 1e3, 700)
    eng.set_frames([p], None)
    for degree in (2, 3):
        want = smoothref.smooth(p, 16, 0.0, None, degree, 0.0)
        assert want["moved"].all()
        assert_same(eng.smooth_points(0, 16, 0.0, None, degree), want, ("scale 1e-3 offset 1e3", degree), KEYS)


def test_max_nn_below_the_basis_moves_nothing(eng):
    p = jetcases.blob()
    eng.set_frames([p], None)
    for k, degree in ((5, 2), (9, 3)):
        got = eng.smooth_points(0, k, 0.0, jetcases.VIEWPOINT, degree)
        assert (got["used"] == k).all() and not got["moved"].any() and not got["shift"].any() and not got["H"].any() and not got["K"].any()
        assert got["xyz"].tobytes() == p.tobytes()
        assert_same(got, smoothref.smooth(p, k, 0.0, jetcases.VIEWPOINT, degree, 0.0), ("max_nn < M", k, degree), KEYS)


def test_tiny_clouds(eng):
    rng = np.random.default_rng(4)
    p12, p2, p0 = rng.normal(0, 0.2, (12, 3)), rng.normal(0, 0.2, (2, 3)), np.zeros((0, 3))
    eng.set_frames([p12, p2, p0], None)
    want = smoothref.smooth(p12, 64, 0.0, None, 3, 0.0)
    assert (want["used"] == 12).all()
    assert_same(eng.smooth_points(0, 64, 0.0, None, 3), want, "n = 12 at max_nn = 64", KEYS)
    want = smoothref.smooth(p2, 16, 0.0, None, 2, 0.0)
    assert (want["used"] == 2).all() and not want["moved"].any()
    assert_same(eng.smooth_points(1, 16, 0.0, None, 2), want, "n = 2", KEYS)
    for device in (False, True):
        got = eng.smooth_points(2, 16, 0.0, None, 3, device=device)
        assert tuple(got["xyz"].shape) == (0, 3) and tuple(got["moved"].shape) == (0,) and tuple(got["nrm"].shape) == (0, 3)
    assert eng.lib.mvicp_smooth_fetch(eng.h, 0, None, None, None, None, None) == 0


def test_a_limit_on_the_shift(eng, blob_ref):
    p, k, r, vp, degree = CASES["blob-16-3"]
    limit = float(np.median(np.abs(blob_ref["shift"])))      # about 0.032
    want = smoothref.smooth(p, k, r, vp, degree, limit)
    fitted, moved = want["fitted"].astype(bool), want["moved"].astype(bool)
    assert (fitted & moved).sum() > 50 and (fitted & ~moved).sum() > 50
    assert want["shift"].tobytes() == blob_ref["shift"].tobytes()      # the shift is reported either way
    eng.set_frames([p], None)
    assert_same(eng.smooth_points(0, k, r, vp, degree, limit), want, "max_shift at the median |shift|", KEYS)
    # exactly at a row's |shift| the row still moves; +inf and a negative limit are no limit
    edge = float(np.sort(np.abs(blob_ref["shift"]))[100])
    want = smoothref.smooth(p, k, r, vp, degree, edge)
    assert want["moved"].sum() == 101
    assert_same(eng.smooth_points(0, k, r, vp, degree, edge), want, "max_shift equal to a row's |shift|", KEYS)
    for limit in (INF, -1.0, -INF):
        assert_same(eng.smooth_points(0, k, r, vp, degree, limit), blob_ref, ("max_shift", limit), KEYS)


def test_a_device_upload_and_device_destinations(eng):
    p, k, r, vp, degree = CASES["hybrid-3"]
    want = smoothref.smooth(p, k, r, vp, degree, 0.0)
    dev = torch.device("cuda", 0)
    eng.set_frames([p[:10]], None)
    eng.set_frame_device(0, torch.from_numpy(p).to(dev))
    got = eng.smooth_points(0, k, r, vp, degree, device=True)
    assert all(isinstance(got[key], torch.Tensor) and got[key].is_cuda for key, _, _ in KEYS)
    assert_same(got, want, "device upload, device destinations", KEYS)
    # one destination at a time, on the host; a short destination is refused
    host = np.zeros(len(p), np.uint8)
    assert eng.lib.mvicp_smooth_fetch(eng.h, len(p), None, None, host.ctypes.data_as(C.c_void_p), None, None) == 0
    assert host.tobytes() == want["moved"].tobytes()
    K = np.zeros(len(p))
    assert eng.lib.mvicp_smooth_fetch(eng.h, len(p), None, None, None, None, K.ctypes.data_as(C.c_void_p)) == 0 and K.tobytes() == want["K"].tobytes()
    assert eng.lib.mvicp_smooth_fetch(eng.h, len(p) - 1, None, None, host.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG and b"cap_rows" in eng.lib.mvicp_last_error()


def test_a_second_pass_over_the_device_result(eng, blob_ref):
    """device=True -> set_frame_device -> a second pass: smoothref applied twice"""
    p, k, r, vp, degree = CASES["blob-16-3"]
    second = smoothref.smooth(blob_ref["xyz"], k, r, vp, degree, 0.0)
    assert second["moved"].all() and second["xyz"].tobytes() != blob_ref["xyz"].tobytes()
    eng.set_frames([p], None)
    first = eng.smooth_points(0, k, r, vp, degree, device=True)
    eng.set_frame_device(0, first["xyz"], first["nrm"])
    assert_same(eng.smooth_points(0, k, r, vp, degree, device=True), second, "second pass", KEYS)


def test_the_normals_slot_holds_the_fit(eng):
    p, k, r, vp, degree = CASES["hybrid-3"]
    n = len(p)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    eng.set_frames([p], None)
    fit = eng.fit_normals(0, k, r, vp, degree)
    eng.smooth_points(0, k, r, vp, degree)
    nrm, curv, used, flags = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    assert eng.lib.mvicp_normals_fetch(eng.h, n, ptr(nrm), ptr(curv), ptr(used)) == 0 and eng.lib.mvicp_normals_fit_fetch(eng.h, n, ptr(flags)) == 0
    assert_same({"nrm": nrm, "curvature": curv, "used": used, "fitted": flags}, fit, "normals_fetch / normals_fit_fetch after smooth_points")
    # adoption writes the fitted normals into the frame
    eng.adopt_normals()
    stored = eng.get_structure(0, "snor").view(np.float64).reshape(-1, 3)[eng.get_structure(0, "inv").view(np.int32)]
    assert stored.tobytes() == fit["nrm"].tobytes()


def test_refusals_and_the_fit_around_a_smoothing(blob_ref):
    p, k, r, vp, degree = CASES["blob-16-3"]
    n = len(p)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    e = mvicp.Engine(0)
    try:
        lib, h = e.lib, e.h
        xyz, shift, moved, H, K = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.uint8), np.zeros(n), np.zeros(n)
        fetch = lambda: lib.mvicp_smooth_fetch(h, n, ptr(xyz), ptr(shift), ptr(moved), ptr(H), ptr(K))
        assert fetch() == ERR_STATE                      # nothing yet
        assert lib.mvicp_smooth_fetch(None, n, None, None, None, None, None) == ERR_ARG
        assert lib.mvicp_smooth_points(None, 0, 16, 0.0, None, 3, 0.0) == ERR_ARG
        e.set_frames([p], None)
        before = e.fit_normals(0, k, r, vp, degree)
        assert fetch() == ERR_STATE and b"mvicp_smooth_points" in lib.mvicp_last_error()      # a fit is no smoothing
        got = e.smooth_points(0, k, r, vp, degree)
        assert_same(got, blob_ref, "the smoothing", KEYS)
        # a refused call leaves the result fetchable: a NaN limit, a bad degree, and the fit's own refusals
        for args in ((0, 16, 0.0, None, 3, float("nan")), (0, 16, 0.0, None, 1, 0.0), (0, 16, 0.0, None, 4, 0.0), (0, 2, 0.0, None, 3, 0.0),
                     (0, 65, 0.0, None, 3, 0.0), (0, 16, float("nan"), None, 3, 0.0), (-1, 16, 0.0, None, 3, 0.0), (1, 16, 0.0, None, 3, 0.0)):
            assert lib.mvicp_smooth_points(h, *args) == ERR_ARG, args
        bad = np.array([0.0, np.inf, 0.0])
        assert lib.mvicp_smooth_points(h, 0, 16, 0.0, bad.ctypes.data_as(C.POINTER(C.c_double)), 3, 0.0) == ERR_ARG
        assert fetch() == 0
        nrm, curv, used, flags = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        assert lib.mvicp_normals_fetch(h, n, ptr(nrm), ptr(curv), ptr(used)) == 0 and lib.mvicp_normals_fit_fetch(h, n, ptr(flags)) == 0
        assert_same({"xyz": xyz, "shift": shift, "moved": moved, "H": H, "K": K, "nrm": nrm, "curvature": curv, "used": used, "fitted": flags}, blob_ref,
                    "the smoothing after refused calls", KEYS)
        # the fit is what it was, and drops the smoothing result; so does an estimate
        assert_same(e.fit_normals(0, k, r, vp, degree), before, "the fit after a smoothing")
        assert fetch() == ERR_STATE
        e.smooth_points(0, k, r, vp, degree)
        e.estimate_normals(0, k, r, vp)
        assert fetch() == ERR_STATE
        # the result ends with an upload to its frame, like the fit
        e.smooth_points(0, 10, 0.0, None, 2)
        assert fetch() == 0
        e.set_frame(0, p)
        assert fetch() == ERR_STATE and lib.mvicp_normals_fetch(h, n, ptr(nrm), None, None) == ERR_STATE
    finally:
        e.close()
