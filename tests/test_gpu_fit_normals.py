"""mvicp_fit_normals / mvicp_normals_fit_fetch on the MI355X: nrm, curvature, used and fitted equal the numpy statement of the contract
(tests/jetref.py) byte for byte, signs of zeros included; no tolerance anywhere.  What a case must contain (failed pivots, h == 0, rows
shorter than the basis) is asserted on the reference alone.  Then the slot the result lives in: the fit takes the place of the last
estimate for mvicp_normals_fetch, mvicp_normals_adopt and mvicp_orient_normals(source = 1), and mvicp_estimate_normals is what it was."""
import ctypes as C

import numpy as np
import pytest

import jetcases
import jetref
import mvicp
import normcases
import normref
import orientref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
CASES = jetcases.exact_cases()
KEYS = (("nrm", np.float64, 3), ("curvature", np.float64, 1), ("used", np.int32, 1), ("fitted", np.uint8, 1))


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what, keys=KEYS):
    for key, dt, width in keys:
        a = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else got[key]
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(want[key])
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape, (what, key, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            rows = np.unique(bad // width)
            raise AssertionError((what, key, len(bad), len(rows), rows[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), b.reshape(-1)[bad[:4]].tolist()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_reference(eng, name):
    p, k, r, vp, degree = CASES[name]
    want = jetref.fit(p, k, r, vp, degree)
    fitted, M = want["fitted"].astype(bool), jetref.TERMS[degree]
    if name.startswith("blob"):
        assert fitted.all()
    elif name.startswith("lattice"):
        assert (want["used"] == k).all() and (~fitted).sum() >= 6 and fitted.sum() >= 100      # failed pivots next to fits
    elif name.startswith("hybrid"):
        u = want["used"]
        assert (u == 0).sum() == 0 and (u == 1).any() and (u < M).sum() > 50 and (u == k).sum() > 50      # (a row holds its own point)
    else:
        assert (want["used"] == k).all() and not fitted.any()      # duplicates: h == 0; collinear: a zero pivot
    eng.set_frames([p], None)
    assert_same(eng.fit_normals(0, k, r, vp, degree), want, name)


def test_small_scale_away_from_the_origin(eng):
    p = normcases.placed("blob", 1e-3, 1e3, 700)
    eng.set_frames([p], None)
    for degree in (2, 3):
        want = jetref.fit(p, 16, 0.0, None, degree)
        assert want["fitted"].all()
        assert_same(eng.fit_normals(0, 16, 0.0, None, degree), want, ("scale 1e-3 offset 1e3", degree))


def test_max_nn_below_the_basis_falls_back_everywhere(eng):
    p = jetcases.blob()
    eng.set_frames([p], None)
    for k, degree in ((5, 2), (9, 3)):
        est = eng.estimate_normals(0, k, 0.0, jetcases.VIEWPOINT)
        got = eng.fit_normals(0, k, 0.0, jetcases.VIEWPOINT, degree)
        assert (est["used"] == k).all() and not got["fitted"].any()
        assert_same(got, est, ("max_nn < M", k, degree), KEYS[:3])
        assert_same(got, jetref.fit(p, k, 0.0, jetcases.VIEWPOINT, degree), ("max_nn < M against the reference", k, degree))


def test_tiny_clouds(eng):
    rng = np.random.default_rng(4)
    p12, p2, p0 = rng.normal(0, 0.2, (12, 3)), rng.normal(0, 0.2, (2, 3)), np.zeros((0, 3))
    eng.set_frames([p12, p2, p0], None)
    want = jetref.fit(p12, 64, 0.0, None, 3)
    assert (want["used"] == 12).all()
    assert_same(eng.fit_normals(0, 64, 0.0, None, 3), want, "n = 12 at max_nn = 64")
    want = jetref.fit(p2, 16, 0.0, None, 2)
    assert (want["used"] == 2).all() and not want["nrm"].any() and not want["fitted"].any()
    assert_same(eng.fit_normals(1, 16, 0.0, None, 2), want, "n = 2")
    for device in (False, True):
        got = eng.fit_normals(2, 16, 0.0, None, 3, device=device)
        assert tuple(got["nrm"].shape) == (0, 3) and tuple(got["fitted"].shape) == (0,)
    assert eng.lib.mvicp_normals_fit_fetch(eng.h, 0, None) == 0


def test_a_device_upload_and_device_destinations(eng):
    p, k, r, vp, degree = CASES["hybrid-3"]
    want = jetref.fit(p, k, r, vp, degree)
    dev = torch.device("cuda", 0)
    eng.set_frames([p[:10]], None)
    eng.set_frame_device(0, torch.from_numpy(p).to(dev))
    got = eng.fit_normals(0, k, r, vp, degree, device=True)
    assert all(isinstance(got[key], torch.Tensor) and got[key].is_cuda for key, _, _ in KEYS)
    assert_same(got, want, "device upload, device destinations")
    host = np.zeros(len(p), np.uint8)
    assert eng.lib.mvicp_normals_fit_fetch(eng.h, len(p), host.ctypes.data_as(C.c_void_p)) == 0
    assert host.tobytes() == want["fitted"].tobytes()
    assert eng.lib.mvicp_normals_fit_fetch(eng.h, len(p) - 1, host.ctypes.data_as(C.c_void_p)) == ERR_ARG and b"cap_rows" in eng.lib.mvicp_last_error()


def test_refusals_and_the_estimate_around_a_fit():
    p = jetcases.blob()
    n = len(p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    e = mvicp.Engine(0)
    try:
        lib, h = e.lib, e.h
        flags = np.zeros(n, np.uint8)
        assert lib.mvicp_normals_fit_fetch(h, n, vp(flags)) == ERR_STATE                      # nothing yet
        assert lib.mvicp_normals_fit_fetch(None, n, vp(flags)) == ERR_ARG and lib.mvicp_fit_normals(None, 0, 16, 0.0, None, 3) == ERR_ARG
        e.set_frames([p], None)
        before = e.estimate_normals(0, 16, 0.0, jetcases.VIEWPOINT)
        assert_same(before, normref.normals(p, 16, 0.0, jetcases.VIEWPOINT), "estimate before a fit", KEYS[:3])
        assert lib.mvicp_normals_fit_fetch(h, n, vp(flags)) == ERR_STATE and b"mvicp_fit_normals" in lib.mvicp_last_error()   # an estimate is no fit
        fit = e.fit_normals(0, 16, 0.0, jetcases.VIEWPOINT, 3)
        assert_same(fit, jetref.fit(p, 16, 0.0, jetcases.VIEWPOINT, 3), "the fit")
        # a refused call leaves the fit fetchable: a bad degree, and the estimate's own refusals
        for args in ((0, 16, 0.0, None, 1), (0, 16, 0.0, None, 4), (0, 16, 0.0, None, 0), (0, 2, 0.0, None, 3), (0, 65, 0.0, None, 3),
                     (0, 16, float("nan"), None, 3), (-1, 16, 0.0, None, 3), (1, 16, 0.0, None, 3)):
            assert lib.mvicp_fit_normals(h, *args) == ERR_ARG, args
        bad = np.array([0.0, np.inf, 0.0])
        assert lib.mvicp_fit_normals(h, 0, 16, 0.0, bad.ctypes.data_as(C.POINTER(C.c_double)), 3) == ERR_ARG
        nrm, curv, used = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
        assert lib.mvicp_normals_fetch(h, n, vp(nrm), vp(curv), vp(used)) == 0 and lib.mvicp_normals_fit_fetch(h, n, vp(flags)) == 0
        assert_same({"nrm": nrm, "curvature": curv, "used": used, "fitted": flags}, fit, "the fit after refused calls")
        # the estimate is what it was, and takes the slot back
        after = e.estimate_normals(0, 16, 0.0, jetcases.VIEWPOINT)
        assert_same(after, before, "estimate after a fit", KEYS[:3])
        assert lib.mvicp_normals_fit_fetch(h, n, vp(flags)) == ERR_STATE
        # the fit ends with an upload to its frame, like the estimate
        e.fit_normals(0, 10, 0.0, None, 2)
        e.set_frame(0, p)
        assert lib.mvicp_normals_fit_fetch(h, n, vp(flags)) == ERR_STATE and lib.mvicp_normals_fetch(h, n, vp(nrm), None, None) == ERR_STATE
    finally:
        e.close()


def test_adopt_and_orient_act_on_the_fit(eng):
    p = jetcases.blob()
    eng.set_frames([p], None)
    fit = eng.fit_normals(0, 16, 0.0, jetcases.VIEWPOINT, 3)
    want = jetref.fit(p, 16, 0.0, jetcases.VIEWPOINT, 3)
    assert_same(fit, want, "the fit")
    # source = 1 reads the fitted normals
    got = eng.orient_normals(0, 10, 0.0, source=1)
    ref = orientref.orient(p, want["nrm"], 10, 0.0)
    assert got["components"] == ref["components"] and orientref.same(got, ref)
    assert not orientref.same(ref, orientref.orient(p, normref.normals(p, 16, 0.0, jetcases.VIEWPOINT)["nrm"], 10, 0.0))   # (not the PCA normals')
    # adoption leaves the frame's normals equal to the fit
    assert eng.get_structure(0, "snor").size == 0
    eng.adopt_normals()
    stored = eng.get_structure(0, "snor").view(np.float64).reshape(-1, 3)[eng.get_structure(0, "inv").view(np.int32)]
    assert stored.tobytes() == want["nrm"].tobytes()
    assert_same(eng.fit_normals(0, 16, 0.0, jetcases.VIEWPOINT, 3), want, "a fit on a frame that has normals")
