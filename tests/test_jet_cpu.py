"""CPU (-m "not gpu"): the contract of mvicp_fit_normals (tests/jetref.py).  Its two forms give the same bytes; a refused fit keeps the bytes of
mvicp_estimate_normals; a plane and a paraboloid come back to rounding; on the bump surface the cubic fit removes most of the PCA normal's
error; and a symmetric registration over fitted normals ends closer to the truth than over PCA normals."""
import numpy as np
import pytest

import initref
import jetcases
import jetref
import matchref
import normcases
import normref
import symref
from test_normals_cpu import VIEW
from test_sym_cpu import host_registration

CASES = jetcases.exact_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_equals_vectorised(name):
    p, k, r, vp, degree = CASES[name]
    a, b = jetref.fit(p, k, r, vp, degree), jetref.fit_loop(p, k, r, vp, degree)
    assert jetref.same(a, b)
    M, fitted = jetref.TERMS[degree], a["fitted"].astype(bool)
    print("JET %s: %d of %d rows fitted, %d with fewer than %d entries" % (name, fitted.sum(), len(p), (a["used"] < M).sum(), M))
    if name.startswith("blob"):
        assert fitted.all()
    if name.startswith("lattice"):      # singular neighbourhoods whose pivots are zero or rounding noise
        assert (a["used"] == k).all() and (~fitted).any() and fitted.any()
    if name.startswith("hybrid"):
        assert (a["used"] < M).any() and (a["used"] == k).any()


@pytest.mark.parametrize("name", ["hybrid-2", "hybrid-3", "duplicates", "collinear"])
def test_fallback_rows_are_the_estimate(name):
    p, k, r, vp, degree = CASES[name]
    got, pca = jetref.fit(p, k, r, vp, degree), normref.normals(p, k, r, vp)
    assert got["curvature"].tobytes() == pca["curvature"].tobytes() and got["used"].tobytes() == pca["used"].tobytes()
    back = got["fitted"] == 0
    assert got["nrm"][back].tobytes() == pca["nrm"][back].tobytes()
    if name.startswith("hybrid"):
        assert (back == (got["used"] < jetref.TERMS[degree])).all()      # a blob's full-enough rows all pass
        assert (got["nrm"][~back] != pca["nrm"][~back]).any(axis=1).all()
    else:
        assert (got["used"] == k).all() and back.all()      # h == 0 / a zero pivot, not a short row


@pytest.mark.parametrize("degree", [2, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_plane_in_general_position(seed, degree):
    p, nrm = jetcases.plane(seed)
    got = jetref.fit(p, 16, 0.0, None, degree)
    ang = np.radians(jetref.angle_deg(got["nrm"], np.broadcast_to(nrm, got["nrm"].shape)))
    print("JET plane seed=%d degree=%d: largest angle %.2e rad, %d of %d rows fitted" % (seed, degree, ang.max(), got["fitted"].sum(), len(p)))
    assert ang.max() <= 1e-12


@pytest.mark.parametrize("degree", [2, 3])
def test_a_paraboloid_is_inside_the_model(degree):
    """Measured with this file's reference: see the print.  The window is jetcases.paraboloid's, where the reason for its size is written
    down; over a window of half-width 1 the same surface is reproduced to (kappa r)^2 only, which the second print shows."""
    p, nrm = jetcases.paraboloid()
    got = jetref.fit(p, 16, 0.0, (0.0, 0.0, 1.0), degree)
    fitted = got["fitted"].astype(bool)
    ang = np.radians(jetref.angle_deg(got["nrm"], nrm))
    pca = np.radians(jetref.angle_deg(normref.normals(p, 16, 0.0, (0.0, 0.0, 1.0))["nrm"], nrm))
    print("JET paraboloid degree=%d: %d of %d rows fitted, largest angle %.2e rad (PCA: largest %.2e, median %.2e)" % (
        degree, fitted.sum(), len(p), ang[fitted].max(), pca.max(), np.median(pca)))
    wide_p, wide_n = jetcases.paraboloid(half_width=1.0)
    wide = np.radians(jetref.angle_deg(jetref.fit(wide_p, 16, 0.0, (0.0, 0.0, 1.0), degree)["nrm"], wide_n))
    print("JET paraboloid degree=%d over half-width 1 (not asserted): largest angle %.2e rad, median %.2e" % (degree, wide.max(), np.median(wide)))
    assert fitted.any() and ang[fitted].max() <= 1e-9
    assert pca.max() > 1e-9


@pytest.fixture(scope="module")
def bump_errors():
    p, nrm = matchref.bumps(1500, 100)
    rows = normref.normals(p, 16, 0.0, None)
    out = {0: (jetref.angle_deg(rows["nrm"], nrm), None)}
    for degree in (2, 3):
        got = jetref.fit(p, 16, 0.0, None, degree, rows["knn"])
        out[degree] = (jetref.angle_deg(got["nrm"], nrm), got["fitted"])
    return out


def test_accuracy_on_the_bump_surface(bump_errors):
    """matchref.bumps(1500, 100), k = 16, degrees to the analytic normal up to sign.  A numpy prototype with ordinary summation: PCA median
    3.35 / mean 4.39, degree 2 2.08 / 3.11, degree 3 0.47 / 0.84."""
    for degree in (0, 2, 3):
        e = bump_errors[degree][0]
        print("JET bumps %s: median %.3f mean %.3f p95 %.3f deg" % ("PCA" if degree == 0 else "degree %d" % degree, np.median(e), e.mean(), np.percentile(e, 95)))
    pca, d2, d3 = bump_errors[0][0], bump_errors[2][0], bump_errors[3][0]
    assert bump_errors[2][1].all() and bump_errors[3][1].all()
    assert d3.mean() <= 0.5 * pca.mean() and np.median(d3) <= 0.25 * np.median(pca)
    assert d2.mean() < pca.mean()


def test_accuracy_on_every_view_of_the_fixture():
    """initref.fixture_clouds(), degree 3 at k = 16: mean error per view at most half the PCA normal's (the prototype: at most 0.21 x)"""
    fx = initref.fixture_clouds()
    for view, (p, nrm) in enumerate(zip(fx["xyz"], fx["nrm"])):
        rows = normref.normals(p, 16, 0.0, None)
        got = jetref.fit(p, 16, 0.0, None, 3, rows["knn"])
        pca, fit = jetref.angle_deg(rows["nrm"], nrm).mean(), jetref.angle_deg(got["nrm"], nrm).mean()
        print("JET fixture view %d: mean %.3f deg (PCA %.3f), %d rows fell back" % (view, fit, pca, (got["fitted"] == 0).sum()))
        assert fit <= 0.5 * pca


def with_normals(cl, make):
    """the clouds of matchref.e2e_clouds with make(points, viewpoint) in place of the analytic normals; the viewpoints are those of
    test_normals_cpu.estimated"""
    out = dict(cl)
    view_dst = cl["truth"][:3, :3] @ VIEW + cl["truth"][:3, 3]
    out["src_nrm"], out["dst_nrm"] = make(cl["src"], VIEW), make(cl["dst"], view_dst)
    return out


@pytest.mark.parametrize("partial", [False, True])
def test_symmetric_registration_gains_from_the_fit(partial):
    """host_registration (tests/test_sym_cpu.py) over degree-3 normals at k = 16 against the same over PCA normals.  A numpy prototype:
    full overlap 0.0047 deg / 0.0125 spacings against 0.0104 / 0.0232, partial 0.0120 / 0.0192 against 0.0194 / 0.0558.  Point-to-plane is
    printed, not asserted: it does not gain consistently."""
    cl = matchref.e2e_clouds(partial)
    sets = {"PCA": with_normals(cl, lambda p, vp: normref.normals(p, 16, 0.0, vp)["nrm"]),
            "degree 3": with_normals(cl, lambda p, vp: jetref.fit(p, 16, 0.0, vp, 3)["nrm"])}
    got = {}
    for name, c in sets.items():
        for symmetric in (False, True):
            got[name, symmetric] = symref.distance_to_truth(host_registration(c, symmetric), cl["truth"], cl["src"], cl["spacing"])
            print("JET registration partial=%s %s normals, %s: ends %.4f deg, %.4f spacings" % (
                partial, name, "symmetric" if symmetric else "point-to-plane", got[name, symmetric][0], got[name, symmetric][1]))
    assert got["degree 3", True][0] < got["PCA", True][0] and got["degree 3", True][1] < got["PCA", True][1], got
