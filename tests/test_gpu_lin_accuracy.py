"""-m gpu: conditioning sweep of linearize_kernel + reduce_expand_kernel (csrc/linearize.hip) against the extended-precision reference
of tests/xprec.py.

Two-frame, one-edge problems (tests/lincases.py) with explicit lists, plus one searched route per family (an identity list:
the kernel then reads p from the shared sorted source cloud).  Point-to-plane and point-to-point, robust on and off, through mvicp_linearize
and both slots of mvicp_linearize_pair.  Error measure: for each of the 10 upper 3x3 sub-blocks of H, each of the 4 three-vectors of g, and
the cost, max|got - xref| / max|xref| WITHIN that piece; where xref is exactly zero, got must be exactly zero.  Bar: the fp64 oracle's own
error on the same piece of the same case (orc.edge_blocks against the same reference), floored at 2^-52, times MARGIN = 32 — the GPU's
association order (per-lane serial, LDS tree, chunk partials) differs from the oracle's serial sum, a lost digit and a half does not fit.
tests/test_xprec.py checks on the CPU that the oracle's error on these cases is what rounding analysis predicts.

Every case prints its worst ratio; the table is in DESIGN.md section 7."""
import numpy as np
import pytest

import lincases
import mvicp
import xprec
from mvicp import synth

pytestmark = pytest.mark.gpu

MARGIN = 32.0
FLAGS = [(1, 1), (1, 0), (0, 1), (0, 0)]   # (point_to_plane, robust)
_REF_CACHE = {}


def _second_poses(poses, seed=11):
    """another pose set a small step away (the other slot of a paired launch)"""
    rng = np.random.default_rng(seed)
    return np.array([synth.add_noise(P, 2e-3, 1e-3, rng) for P in poses])


def _engine(case):
    eng = mvicp.Engine(0)
    if case["chunk"]:
        eng.set_option("lin_chunk", case["chunk"])    # takes effect at set_graph
    eng.set_frames([case["dst"], case["src"]], [case["nor"], case["nor"]])
    eng.set_graph([1], [0])
    return eng


def _references(orc, case, first, second, a, key):
    """{(plane, robust): (xref, oracle's piece errors)}; key = None: not cached (the 1 000 001-point case is, for both chunk sizes)"""
    if key is None or key not in _REF_CACHE:
        p, q, n = lincases.gathered(case, first, second)
        out = {}
        for plane, robust in FLAGS:
            ref = xprec.edge_block(p, q, n, case["poses"][1], case["poses"][0], a, plane, robust)
            out[(plane, robust)] = (ref, xprec.piece_errors(xprec.unpack(lincases.oracle_block(orc, case, plane, robust, first, second, a)), ref))
        if key is None:
            return out
        _REF_CACHE[key] = out
    return _REF_CACHE[key]


def _cost_bar(case, first, second, a, plane):
    """What fp64 allows the robust cost rho / 2 = s w / (1 + w) summed over the correspondences, relative to the sum — from the number format and
    the data alone, not from any implementation.  The residual is a difference of coordinates of size E = max|p| + max|q| + |t_rel| + |t_s| + |t_d|
    (the frame-local points, the relative and the two world translations the relative transform is rounded from); a dozen roundings of that size
    (the rotation, the dot product or the three differences, c = n . q, the relative transform itself) bound its error by dr = 8 eps E.
    d(rho / 2) / dr = w r, so the sum moves by at most dr sum w |r| if every error pulls the same way, plus 16 eps of the sum for the evaluation
    of w, of s w / (1 + w) and for the summation tree.  The textbook form a^2 (sqrt(1 + s / a^2) - 1) does not meet this for a >> |r|: it rounds
    every term to an ulp of a^2 (1e-4 of the term at a = 1e6 |r|)."""
    p, q, n = lincases.gathered(case, first, second)
    Pd, Ps = case["poses"]
    Rel = np.linalg.inv(Pd) @ Ps
    f = p @ Rel[:3, :3].T + Rel[:3, 3] - q
    r = np.abs(np.sum(f * n, axis=1)) if plane else np.linalg.norm(f, axis=1)
    w = 1.0 / np.sqrt(1.0 + (r / float(a)) ** 2)
    half_rho = np.sum(r * r * w / (1.0 + w))
    E = np.abs(p).max() + np.abs(q).max() + np.linalg.norm(Rel[:3, 3]) + np.linalg.norm(Pd[:3, 3]) + np.linalg.norm(Ps[:3, 3])
    eps = 2.0 ** -52
    return (8 * eps * E * np.sum(w * r) + 16 * eps * half_rho) / half_rho


def _sweep_one(eng, orc, case, first, second, a, key, label, pin_cost=False):
    refs = _references(orc, case, first, second, a, key)
    P = case["poses"]
    P2 = _second_poses(P)
    failures = []
    for plane, robust in FLAGS:
        ref, err_orc = refs[(plane, robust)]
        single = eng.linearize(P, plane, robust)
        pa, _ = eng.linearize_pair(P, P2, plane, robust)
        _, qb = eng.linearize_pair(P2, P, plane, robust)
        for route, blk in (("linearize", single[0]), ("pair slot 0", pa[0]), ("pair slot 1", qb[0])):
            assert np.all(np.isfinite(blk)), (label, plane, robust, route)
            err = xprec.piece_errors(xprec.unpack(blk), ref)
            ratio, where = xprec.worst_ratio(err, err_orc)
            if route == "linearize":
                oh = max(v for k, v in err_orc.items() if k[0] == "H")
                og = max((v for k, v in err_orc.items() if k[0] == "g" and np.isfinite(v)), default=0.0)
                kh = max(v for k, v in err.items() if k[0] == "H")
                kg = max(v for k, v in err.items() if k[0] == "g")
                print("SWEEP %-34s plane=%d robust=%d  oracle H %.1e g %.1e cost %.1e | kernel H %.1e g %.1e cost %.1e | worst ratio %.2f at %s" % (
                    label, plane, robust, oh, og, err_orc["cost"], kh, kg, err["cost"], ratio, where))
            if not ratio <= MARGIN:
                failures.append((label, plane, robust, route, where, ratio, err[where], err_orc[where]))
            if pin_cost and robust:
                bar = _cost_bar(case, first, second, a, plane)
                if route == "linearize":
                    print("COST  %-34s plane=%d  kernel %.1e  fp64 bar %.1e  oracle %.1e" % (label, plane, err["cost"], bar, err_orc["cost"]))
                if not err["cost"] <= bar:
                    failures.append((label, plane, robust, route, "cost against the fp64 bar", err["cost"], bar))
    return failures


def _run_explicit(orc, name, kw, pin_cost):
    case = lincases.make_case(name, **kw)
    eng = _engine(case)
    try:
        eng.set_correspondences(0, case["first"], case["second"], case["a"])
        return _sweep_one(eng, orc, case, case["first"], case["second"], case["a"], None, name, pin_cost)
    finally:
        eng.close()


@pytest.mark.parametrize("family", list(lincases.FAMILIES))
def test_linearize_conditioning_sweep_explicit_lists(orc, family):
    """every member of one family (lincases.FAMILIES) with explicit correspondences and scale.  The robust-scale family also holds the
    robust cost to an absolute fp64 bar (_cost_bar): at a >> |r| the oracle's own textbook form cancels, so 32 x its error says nothing there"""
    failures = []
    for fam, name, kw in lincases.all_cases():
        if fam == family:
            failures += _run_explicit(orc, name, kw, pin_cost=(family == "a"))
    assert not failures, failures


@pytest.mark.parametrize("family", list(lincases.SEARCHED))
def test_linearize_conditioning_sweep_searched_identity_lists(orc, family):
    """one member per family through mvicp_correspond with a cutoff that accepts every query: the list is the identity, so the kernel takes
    its shared-source-cloud path (p from the sorted cloud, not from the stream); lists and scale are what the search returned.  The zero
    family is searched with the dst frame 2^-12 aside (lincases.make_case), which gives the same identity list with a scale > 0, and
    linearized at the poses where every residual is exactly zero."""
    kw = dict(lincases.SEARCHED[family], seed=900 + len(family))
    name = "searched " + lincases.case_name(family, lincases.SEARCHED[family])
    case = lincases.make_case(name, **kw)
    eng = _engine(case)
    try:
        counts, weights = eng.correspond(case["search_poses"], [1, 0], 100 * lincases.NOISE * kw.get("unit", 1.0))
        assert counts[0] == len(case["src"]), (counts, len(case["src"]))   # every query accepted -> identity list
        first, second, _ = eng.get_correspondences(0)
        assert np.array_equal(first, np.arange(len(case["src"])))
        failures = _sweep_one(eng, orc, case, first, second, weights[0], None, name)
    finally:
        eng.close()
    assert not failures, failures


@pytest.fixture(scope="module")
def big_case():
    return lincases.make_case("count:N=1000001", seed=4242, N=1000001)


@pytest.mark.parametrize("chunk", [kw["chunk"] for kw in lincases.BIG])
def test_linearize_conditioning_sweep_a_million_correspondences(orc, big_case, chunk):
    """N = 1 000 001 (odd; 977 / 123 chunk partials per edge for reduce_expand_kernel to sum), the cloud and the references built once"""
    case = dict(big_case, chunk=chunk)
    eng = _engine(case)
    try:
        eng.set_correspondences(0, case["first"], case["second"], case["a"])
        failures = _sweep_one(eng, orc, case, case["first"], case["second"], case["a"], "big", "count:N=1000001,chunk=%d" % chunk)
    finally:
        eng.close()
    assert not failures, failures
