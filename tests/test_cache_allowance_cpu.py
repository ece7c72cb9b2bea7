"""The rounding allowance of the temporal cache (mvicp_cache_allowance) against the measured error of the fp64 query
map.  No GPU: tests/offorigin.py restates xf_point operation by operation in numpy, once in float64 and once in np.longdouble.

The map rounds g = R p + ts at the size of ts, so two poses that share a large world translation (georeferenced scans) have a small
relative translation v and still an error of 2^-53 |ts|; the allowance must follow |ts| and |td|, not |v|."""
import numpy as np
import pytest

import mvicp
import offorigin as oo

assert np.finfo(oo.LD).nmant >= 63, "np.longdouble has no 64-bit significand on this platform: the extended-precision map is not available"

TS = [0.0, 1.0, 1e2, 1e4, 1e6, 4e6, 1e8]
RMAX = [1e-3, 0.1, 1e3]
N = 20000


def _case(T, rmax, unequal, seed):
    """Old and new pose pair (one small step of the source pose in between) and a cloud with max |p| <= rmax."""
    rng = np.random.default_rng(seed)
    W = T * np.array([1.0, -0.7, 0.3])
    ts = W + rng.normal(0, 0.05, 3)
    td = W + rng.normal(0, 0.05, 3) + (oo.DU3 if unequal else 0.0)
    Ps = oo.pose(oo.random_rotation(rng), ts); Pd = oo.pose(oo.random_rotation(rng), td)
    Ps2 = Ps @ oo.small_motion(rng, 1e-9)
    p = rng.uniform(-1, 1, (N, 3)) * (rmax / np.sqrt(3.0))
    return Ps, Pd, Ps2, p


CASES = [(T, r, uq) for T in TS for r in RMAX for uq in (False, True)]


@pytest.fixture(scope="module")
def measured():
    """Per case: (allowance, err(P_old) + err(P_new), the parent's formula, |ts| + |td|)."""
    out = {}
    for i, (T, rmax, uq) in enumerate(CASES):
        Ps, Pd, Ps2, p = _case(T, rmax, uq, 700 + i)
        r = float(np.linalg.norm(p, axis=1).max())
        b_old, b_new = oo.query_block(Ps, Pd), oo.query_block(Ps2, Pd)
        err = oo.xf_error(b_old, p) + oo.xf_error(b_new, p)
        out[(T, rmax, uq)] = (mvicp.cache_allowance(Ps, Pd, Ps2, Pd, r), err, oo.parent_allowance(b_new, r),
                              float(np.linalg.norm(Ps2[:3, 3]) + np.linalg.norm(Pd[:3, 3])))
    return out


def test_allowance_covers_both_evaluations_of_the_query_map(measured):
    """allowance >= 2 (err(P_old) + err(P_new)): twice, because a random sweep does not find the worst rounding."""
    worst = 0.0
    for key, (allow, err, _, _) in measured.items():
        worst = max(worst, 2.0 * err / allow)
        assert allow >= 2.0 * err, (key, allow, err)
    print("worst 2 (err_old + err_new) / allowance over %d cases of %d points: %.3g" % (len(measured), N, worst))


def test_allowance_stays_within_the_limit_over_the_parents_formula(measured):
    """No more than the parent's value plus its own 1e-12 convention applied to the terms it forgot, 4e-12 (|ts| + |td|): "no cache hits
    away from the origin" is not a fix."""
    for key, (allow, _, parent, tnorm) in measured.items():
        assert 0.0 < allow <= parent + 4e-12 * tnorm, (key, allow, parent, tnorm)


def test_parents_formula_fails_far_from_the_origin(measured):
    """What this test is for: the formula it replaced (kept as a literal) does not cover the measured error at T >= 1e6."""
    for (T, rmax, uq), (_, err, parent, _) in measured.items():
        if T >= 1e6 and rmax <= 0.1:     # a small cloud: scale = max(1, |v|), the old value stays at 2e-12 .. 2e-11
            assert parent < 2.0 * err, ((T, rmax, uq), parent, err)
        if T <= 1e2:
            assert parent >= 2.0 * err, ((T, rmax, uq), parent, err)


def test_identical_transforms_give_zero_and_any_change_a_positive_value():
    Ps, Pd, Ps2, p = _case(4e6, 0.1, True, 3)
    assert mvicp.cache_allowance(Ps, Pd, Ps, Pd, 0.1) == 0.0
    assert mvicp.cache_allowance(Ps, Pd, Ps.copy(), Pd.copy(), 1e3) == 0.0
    Pn = Ps.copy(); Pn[0, 3] = np.nextafter(Pn[0, 3], np.inf)
    assert mvicp.cache_allowance(Ps, Pd, Pn, Pd, 0.1) > 0.0
    assert mvicp.cache_allowance(Ps, Pd, Ps, Pd @ oo.small_motion(np.random.default_rng(1), 1e-12), 0.1) > 0.0
    Z = np.zeros((4, 4))
    assert mvicp.cache_allowance(Z, Ps, Ps, Ps, 0.0) > 0.0      # never 0 for transforms that differ, whatever they are


def test_allowance_is_the_documented_formula_and_rejects_bad_arguments(engine_lib):
    import ctypes as C
    from mvicp import lib as L
    Ps, Pd, Ps2, p = _case(1e6, 0.1, True, 4)
    want = 0.0
    for b in (oo.query_block(Ps, Pd), oo.query_block(Ps2, Pd)):
        R, ts, Ri, td = b
        want += np.linalg.norm(Ri) * (np.linalg.norm(ts) + 16.0 * np.linalg.norm(R) * 0.25 + 13.0 * np.linalg.norm(ts - td))
    got = mvicp.cache_allowance(Ps, Pd, Ps2, Pd, 0.25)
    assert abs(got / (2.0 ** -52 * want) - 1.0) < 1e-14
    assert "mvicp_cache_allowance" in L.SYMBOLS
    P = L.poses_to_c(np.stack([Ps, Pd]))
    out = C.c_double(-1.0)
    f = engine_lib.mvicp_cache_allowance
    assert f(L._dp(P[0]), L._dp(P[1]), L._dp(P[0]), L._dp(P[1]), 0.1, None) == -1
    assert f(None, L._dp(P[1]), L._dp(P[0]), L._dp(P[1]), 0.1, C.byref(out)) == -1
    assert f(L._dp(P[0]), L._dp(P[1]), L._dp(P[0]), L._dp(P[1]), -1.0, C.byref(out)) == -1
    assert f(L._dp(P[0]), L._dp(P[1]), L._dp(P[0]), L._dp(P[1]), float("nan"), C.byref(out)) == -1
    assert out.value == -1.0
