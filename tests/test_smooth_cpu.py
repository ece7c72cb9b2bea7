"""CPU (-m "not gpu"): the contract of mvicp_smooth_points (tests/smoothref.py).  Its two forms give the same bytes; its normals are
mvicp_fit_normals'; a plane is not moved and has no curvature; a sphere has the curvatures of a sphere; noise along the normal of the bump
surface shrinks; and a registration of two noisy clouds ends at most half as far from the truth after smoothing."""
import numpy as np
import pytest

import jetcases
import jetref
import mvicp
import smoothcases
import smoothref
import symref
from test_sym_cpu import host_registration

CASES = jetcases.exact_cases()


def splitting_shift(name):
    """the median |shift| of the case's fitted rows: a max_shift that moves about half of them"""
    p, k, r, vp, degree = CASES[name]
    ref = smoothref.smooth(p, k, r, vp, degree, 0.0)
    fitted = ref["fitted"].astype(bool)
    return float(np.median(np.abs(ref["shift"][fitted]))) if fitted.any() else 0.01


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_equals_vectorised(name):
    p, k, r, vp, degree = CASES[name]
    for max_shift in (0.0, splitting_shift(name)):
        a, b = smoothref.smooth(p, k, r, vp, degree, max_shift), smoothref.smooth_loop(p, k, r, vp, degree, max_shift)
        assert smoothref.same(a, b), (name, max_shift)
        fitted, moved = a["fitted"].astype(bool), a["moved"].astype(bool)
        print("SMOOTH %s max_shift=%.4g: %d of %d rows fitted, %d moved, largest |shift| %.4g" % (
            name, max_shift, fitted.sum(), len(p), moved.sum(), np.abs(a["shift"]).max()))
        assert not (moved & ~fitted).any() and a["xyz"][~moved].tobytes() == p[~moved].tobytes()
        assert all(np.isfinite(a[key]).all() for key in ("xyz", "shift", "H", "K"))
        assert not a["shift"][~fitted].any() and not a["H"][~fitted].any() and not a["K"][~fitted].any()
        if max_shift == 0.0:
            assert (moved == fitted).all()
        elif name.startswith("blob"):
            assert moved.sum() > 50 and (fitted & ~moved).sum() > 50


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_normals_are_the_fit(name):
    p, k, r, vp, degree = CASES[name]
    assert jetref.same(smoothref.smooth(p, k, r, vp, degree, 0.0), jetref.fit(p, k, r, vp, degree))


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_plane_is_not_moved_and_is_flat(seed, degree):
    """|a_0| <= 1e-13 and |H| h <= 1e-11 (a prototype: 1.6e-15 and 5.9e-14); h is at most the cloud's extent, so H times the largest
    neighbourhood scale is what is asserted"""
    p, _ = jetcases.plane(seed)
    got = smoothref.smooth(p, 16, 0.0, None, degree, 0.0)
    rows = got["knn"]
    idx = np.maximum(rows["idx"], 0)
    h = np.sqrt(((p[idx] - p[:, None, :]) ** 2).sum(-1).max(axis=1))
    a0, Hh = np.abs(got["shift"]) / h, np.abs(got["H"]) * h
    print("SMOOTH plane seed=%d degree=%d: largest |a_0| %.2e, largest |H| h %.2e, %d of %d rows fitted" % (
        seed, degree, a0.max(), Hh.max(), got["fitted"].sum(), len(p)))
    assert got["fitted"].all() and got["moved"].all()
    assert a0.max() <= 1e-13 and Hh.max() <= 1e-11


@pytest.mark.parametrize("degree", [2, 3])
def test_a_sphere_has_the_curvatures_of_a_sphere(degree):
    """smoothcases.sphere(): 331 points on a sphere of R = 2, max_nn 16.  Seen from its centre the normals point inwards and the surface
    bends towards them: H = +1/R; seen from outside H = -1/R, the same bytes negated.  K = 1/R^2 either way.  Asserted at degree 2: H within
    3 %, K within 5 % (a prototype: 1.0 % and 2.1 %); degree 3 is printed (a prototype: 1.6 % and 3.1 %)."""
    R, centre = 2.0, np.array([0.3, -0.2, 0.5])
    p = smoothcases.sphere(10, 0.1, R, centre)
    assert len(p) == 331
    got = smoothref.smooth(p, 16, 0.0, centre, degree, 0.0)
    assert got["fitted"].all() and got["moved"].all()
    hr, kr = got["H"] * R, got["K"] * R * R
    off = np.abs(np.linalg.norm(got["xyz"] - centre, axis=1) - R)
    print("SMOOTH sphere degree=%d: H R in [%.4f, %.4f], K R^2 in [%.4f, %.4f], projected points within %.2e of the sphere" % (
        degree, hr.min(), hr.max(), kr.min(), kr.max(), off.max()))
    out = smoothref.smooth(p, 16, 0.0, centre + np.array([0.0, 0.0, 100.0]), degree, 0.0)
    assert (out["H"] < 0).all() and (out["K"] > 0).all()
    # the principal curvatures: their mean is H, and their product is K wherever H H >= K (an umbilic point may round to H H < K)
    k1, k2 = mvicp.principal_curvatures(got["H"], got["K"])
    real = got["H"] * got["H"] >= got["K"]
    assert (k1 >= k2).all() and np.allclose(0.5 * (k1 + k2), got["H"], rtol=1e-14, atol=0) and np.allclose((k1 * k2)[real], got["K"][real], rtol=1e-12, atol=0)
    if degree == 2:
        assert np.abs(hr - 1.0).max() <= 0.03 and np.abs(kr - 1.0).max() <= 0.05
        assert np.abs(out["H"] * R + 1.0).max() <= 0.03 and np.abs(out["K"] * R * R - 1.0).max() <= 0.05


def test_principal_curvatures():
    """D = H H - K, a negative D counts as 0, r = sqrt(D) -> (H + r, H - r)"""
    H, K = np.array([-0.5, 0.5, 0.0, 1.0, 2.0]), np.array([0.25, 0.25, -4.0, 1.0 + 1e-12, 3.0])
    k1, k2 = mvicp.principal_curvatures(H, K)
    assert k1.tolist() == [-0.5, 0.5, 2.0, 1.0, 3.0] and k2.tolist() == [-0.5, 0.5, -2.0, 1.0, 1.0]
    # a cylinder of radius 4 along x seen from inside: curvatures (1/4, 0)
    k1, k2 = mvicp.principal_curvatures(0.125, 0.0)
    assert float(k1) == 0.25 and float(k2) == 0.0


NOISE_TABLE = ((0.5, 30, 2), (0.5, 30, 3), (0.25, 30, 3), (0.25, 16, 2), (0.0, 16, 3), (0.0, 30, 2))


def test_noise_along_the_normal_shrinks():
    """matchref.bumps(1500, 100) with Gaussian noise along the analytic normal, sigma in point spacings; RMS distance to the surface before
    and after, in spacings.  A numpy prototype: sigma 0.5 at (30, 2) 0.491 -> 0.216, at (30, 3) 0.491 -> 0.230; sigma 0.25 at (30, 3) 0.246
    -> 0.129, at (16, 2) 0.246 -> 0.136; the clean cloud at (16, 3) 0 -> 0.015, at (30, 2) 0 -> 0.102 (over-smoothing, as expected)."""
    got = {}
    for sigma, k, degree in NOISE_TABLE:
        p, spacing = smoothcases.noisy_bumps(sigma)
        res = smoothref.smooth(p, k, 0.0, None, degree, 0.0)
        before, after = smoothcases.rms(smoothcases.surface_distance(p)) / spacing, smoothcases.rms(smoothcases.surface_distance(res["xyz"])) / spacing
        got[sigma, k, degree] = (before, after)
        print("SMOOTH bumps sigma=%.2f max_nn=%d degree=%d: RMS distance %.3f -> %.3f spacings, %d rows fell back" % (
            sigma, k, degree, before, after, (res["fitted"] == 0).sum()))
        assert res["fitted"].all() and res["moved"].all()
    for key in ((0.5, 30, 2), (0.5, 30, 3)):
        assert got[key][1] <= 0.6 * got[key][0], (key, got[key])
    assert got[0.0, 16, 3][1] <= 0.03, got[0.0, 16, 3]


def assert_smoothing_halves_the_error(got):
    """got: {(smoothed, symmetric): (degrees, spacings from the truth)}"""
    for symmetric in (False, True):
        raw, smo = got[False, symmetric], got[True, symmetric]
        assert smo[0] <= 0.5 * raw[0] and smo[1] <= 0.5 * raw[1], (symmetric, raw, smo)


@pytest.mark.parametrize("partial", [False, True])
def test_registration_gains_from_smoothing(partial):
    """host_registration (tests/test_sym_cpu.py) on the noisy sigma-0.5 pair of smoothcases.noisy_pair, raw and smoothed first at (30, 2), on
    normals fitted at (16, 3), point-to-plane and symmetric.  A numpy prototype, degrees / spacings from the truth, raw -> smoothed: full
    overlap point-to-plane 0.523 / 0.826 -> 0.075 / 0.085, symmetric 0.343 / 0.684 -> 0.109 / 0.148; partial point-to-plane 0.742 / 1.469
    -> 0.119 / 0.128, symmetric 0.703 / 1.054 -> 0.116 / 0.152.  Asserted: the smoothed run ends at most half as far."""
    cl = smoothcases.noisy_pair(partial)
    got = {}
    for smoothed in (False, True):
        c = dict(cl)
        if smoothed:
            for key, view in (("src", "view_src"), ("dst", "view_dst")):
                c[key] = smoothref.smooth(cl[key], smoothcases.SMOOTH_NN, 0.0, cl[view], smoothcases.SMOOTH_DEGREE, 0.0)["xyz"]
        for key, view in (("src", "view_src"), ("dst", "view_dst")):
            c[key + "_nrm"] = jetref.fit(c[key], smoothcases.FIT_NN, 0.0, cl[view], smoothcases.FIT_DEGREE)["nrm"]
        for symmetric in (False, True):
            got[smoothed, symmetric] = symref.distance_to_truth(host_registration(c, symmetric), cl["truth"], cl["clean_src"], cl["spacing"])
            print("SMOOTH registration (CPU) partial=%s %s, %s: ends %.4f deg, %.4f spacings" % (
                partial, "smoothed" if smoothed else "raw", "symmetric" if symmetric else "point-to-plane", *got[smoothed, symmetric]))
    assert_smoothing_halves_the_error(got)
