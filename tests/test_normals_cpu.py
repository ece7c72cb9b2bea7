"""CPU (-m "not gpu"): the contract of mvicp_estimate_normals (tests/normref.py).  Its two forms give the same bytes; its normals are as
accurate as tests/normcheck.py asks of the recompute_normals kernel (32 x numpy's fp64 route on the same sets) over scales, offsets and
neighbourhood sizes; the degenerate shapes give what the contract says; a viewpoint at the sensor orients every normal of both clouds of
matchref.e2e_clouds to the analytic side; and a registration over ESTIMATED normals keeps the symmetric objective's gain."""
import numpy as np
import pytest

import knnref
import matchref
import normcases
import normcheck
import normref
import symref
from test_sym_cpu import host_registration

VIEW = np.array([0.5, 0.5, 2.0])   # a sensor above the surface of matchref.bumps, in src's coordinates


@pytest.mark.parametrize("case", ["blob", "lattice", "duplicates", "collinear", "hybrid", "short"])
def test_loop_equals_vectorised(case):
    rng = np.random.default_rng(3)
    if case == "blob":
        p, k, r, vp = rng.normal(0, 0.25, (90, 3)), 10, 0.0, (0.1, -0.2, 3.0)
    elif case == "lattice":
        p, k, r, vp = knnref.shuffled_lattice(4), 7, 0.0, None
    elif case == "duplicates":
        p, k, r, vp = normcases.duplicates(8, 8), 12, 0.0, (0.0, 0.0, 1.0)
    elif case == "collinear":
        p, k, r, vp = normcases.collinear(60), 5, 0.0, (1.0, 2.0, 5.0)
    elif case == "hybrid":
        p, k, r, vp = rng.normal(0, 0.25, (90, 3)), 8, 0.25, (0.0, 0.0, 2.0)
    else:
        p, k, r, vp = rng.normal(0, 0.25, (20, 3)), 64, 0.0, (0.0, 0.0, 2.0)
    a, b = normref.normals(p, k, r, vp), normref.normals_loop(p, k, r, vp)
    assert knnref.same(a["knn"], b["knn"])
    assert normref.same(a, b)
    if case == "hybrid":
        assert (a["used"] < 3).any() and (a["used"] == k).any()
        assert not a["nrm"][a["used"] < 3].any() and not a["curvature"][a["used"] < 3].any()


@pytest.mark.parametrize("kind", ["blob", "plane", "lattice", "clusters"])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_accuracy_over_scale_and_offset(kind, scale, offset):
    """normcheck.figures (not normcheck.check, which asserts n_z <= 0): bar 32 x numpy's fp64 route, | |n| - 1 | <= 1e-15.  A numpy
    prototype's worst ratios were 4.3 (Rayleigh) and 2.5 (angle), norm error 2.4e-16; 4, 5, 6 and 8 sweeps gave identical figures."""
    pts = normcases.placed(kind, scale, offset, 1200)
    order, Ds = knnref.sorted_rows(pts)
    for k in (5, 16, 40):
        rows = knnref.from_sorted(order, Ds, k, 0.0)
        got = normref.normals(pts, k, 0.0, None, rows)
        assert np.isfinite(got["nrm"]).all() and np.isfinite(got["curvature"]).all()
        f = normcheck.figures(pts, rows["idx"], got["nrm"])
        r_res = f["res"] / np.maximum(f["res_np"], normcheck.FLOOR)
        r_ang = np.where(f["gap_ok"], f["ang"] / np.maximum(f["ang_np"], normcheck.FLOOR), 0.0)
        print("NORMALS %s scale=%g offset=%g k=%d: Rayleigh ratio %.2f, angle ratio %.2f, norm error %.1e" % (
            kind, scale, offset, k, r_res.max(), r_ang.max(), f["norm_err"].max()))
        assert f["norm_err"].max() <= 1e-15
        assert r_res.max() <= normcheck.MARGIN and r_ang.max() <= normcheck.MARGIN
        assert (got["curvature"] >= 0).all() and (got["curvature"] <= 1.0 / 3.0 + 1e-15).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("value", [0.0, 0.1, -3.3, 1000.1])
def test_a_constant_coordinate_gives_exactly_that_axis(axis, value):
    """the offsets from the point itself cancel the shared coordinate exactly: its row and column of C are zero, no rotation touches them"""
    pts = normcases.constant_coordinate(axis, value)
    e = np.zeros(3); e[axis] = 1.0
    for vp_side in (+1.0, -1.0):
        vp = e * (value + vp_side * 5.0)
        for k in (3, 10, 40):
            got = normref.normals(pts, k, 0.0, vp)
            assert (got["nrm"] == vp_side * e).all()
            assert (got["curvature"] == 0).all() and not np.signbit(got["curvature"]).any()


def test_collinear_and_all_duplicate_neighbourhoods_give_finite_unit_vectors():
    line = normcases.collinear()
    got = normref.normals(line, 10, 0.0, (0.0, 0.0, 10.0))
    assert np.isfinite(got["nrm"]).all() and np.abs(np.linalg.norm(got["nrm"], axis=1) - 1).max() <= 1e-15
    d = np.array([0.25, -0.125, 0.5]); d /= np.linalg.norm(d)
    assert np.abs(got["nrm"] @ d).max() <= 1e-12          # across the line
    dup = normcases.duplicates()
    got = normref.normals(dup, 10, 0.0, (0.0, 0.0, 10.0))
    assert (dup[got["knn"]["idx"]] == dup[:, None, :]).all()      # every neighbourhood is ten copies of its point
    assert np.isfinite(got["nrm"]).all() and np.abs(np.linalg.norm(got["nrm"], axis=1) - 1).max() <= 1e-15
    assert (got["curvature"] == 0).all()


def estimated(cl):
    """the clouds of matchref.e2e_clouds with the contract's normals (k = 16) in place of the analytic ones: the viewpoint is VIEW for src
    and the same point mapped by the truth for dst"""
    out = dict(cl)
    view_dst = cl["truth"][:3, :3] @ VIEW + cl["truth"][:3, 3]
    out["src_nrm"] = normref.normals(cl["src"], 16, 0.0, VIEW)["nrm"]
    out["dst_nrm"] = normref.normals(cl["dst"], 16, 0.0, view_dst)["nrm"]
    return out


@pytest.mark.parametrize("partial", [False, True])
def test_the_sensor_viewpoint_orients_every_normal_to_the_analytic_side(partial):
    cl = matchref.e2e_clouds(partial)
    est = estimated(cl)
    for name in ("src", "dst"):
        dots = (est[name + "_nrm"] * cl[name + "_nrm"]).sum(1)
        print("partial=%s %s: smallest dot product with the analytic normal %.3f" % (partial, name, dots.min()))
        assert (dots > 0).all()
    # the rule this replaces, n_z <= 0 in whatever frame the cloud happens to be expressed in, is no orientation: about half disagree
    wrong = (np.where(est["dst_nrm"][:, 2:3] > 0, -est["dst_nrm"], est["dst_nrm"]) * cl["dst_nrm"]).sum(1) < 0
    print("partial=%s dst by the n_z <= 0 rule: %d of %d on the wrong side" % (partial, wrong.sum(), len(wrong)))


@pytest.mark.parametrize("partial", [False, True])
def test_registration_over_estimated_normals_keeps_the_symmetric_gain(partial):
    """host_registration (tests/test_sym_cpu.py) fed the contract's normals.  Full overlap: the symmetric objective ends closer to the
    truth than point-to-plane in both figures (a numpy prototype: 0.0104 deg / 0.023 spacings against 0.0378 / 0.071).  Partial overlap:
    printed, not asserted (the prototype was mixed: 0.0194 / 0.056 against 0.0117 / 0.081)."""
    cl = estimated(matchref.e2e_clouds(partial))
    got = {}
    for symmetric in (False, True):
        P = host_registration(cl, symmetric)
        got[symmetric] = symref.distance_to_truth(P, cl["truth"], cl["src"], cl["spacing"])
    print("estimated normals, partial=%s  point-to-plane ends %.4f deg, %.4f spacings  |  symmetric ends %.4f deg, %.4f spacings" % (
        partial, got[False][0], got[False][1], got[True][0], got[True][1]))
    if not partial:
        assert got[True][0] < got[False][0] and got[True][1] < got[False][1], got
