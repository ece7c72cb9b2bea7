"""The ISS keypoint contract without a GPU: the numpy reference (tests/issref.py) against a plain Python loop, that it IS Intrinsic Shape
Signatures (an extended-precision covariance and LAPACK's eigenvalues decide every point the same way, up to the points at a
threshold), what the cases contain, the clouds-alone initialisation on keypoints on the CPU, and that the two entry points exist and
reject bad arguments before any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import initref as ir
import issref
import knnref
from mvicp import lib as L

ERR_ARG, ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@pytest.mark.parametrize("name", issref.CASES)
def test_reference_equals_python_loop(name):
    p, args = issref.case(name)
    got, loop = issref.reference(name), issref.iss_loop(p, *args)
    assert issref.same(got, loop)
    assert got["eig"].tobytes() == loop["eig"].tobytes()
    assert 0 < len(got["idx"]) < len(p) and (got["cnt_salient"] >= 1).all() and got["cnt_salient"].max() <= issref.CAP


def test_small_and_degenerate_inputs():
    empty = issref.iss(np.zeros((0, 3)), 0.1, 0.1)
    assert issref.same(empty, issref.iss_loop(np.zeros((0, 3)), 0.1, 0.1)) and len(empty["idx"]) == 0
    rng = np.random.Generator(np.random.PCG64(9))
    for n in (1, 5, 63):
        p = rng.uniform(0.0, 0.05, size=(n, 3))
        got = issref.iss(p, 0.1, 0.1, 0.975, 0.975, 1)
        assert issref.same(got, issref.iss_loop(p, 0.1, 0.1, 0.975, 0.975, 1))
        assert (got["cnt_salient"] == n).all() and (got["cnt_nms"] == n).all()
        assert len(got["idx"]) == (0 if n == 1 else 1)   # (one point: C = 0, l3 = 0; all within one radius: one maximum)
    with pytest.raises(issref.TooManyNeighbours):
        issref.iss(rng.uniform(0.0, 0.01, size=(1100, 3)), 0.1, 0.1)
    for bad in ((0.0, 0.1, 0.9, 0.9, 5), (0.1, float("inf"), 0.9, 0.9, 5), (0.1, 0.1, 0.0, 0.9, 5), (0.1, 0.1, 0.9, float("nan"), 5), (0.1, 0.1, 0.9, 0.9, 0),
                (0.1, 0.1, 0.9, 0.9, 1025), (2.0 ** -301, 0.1, 0.9, 0.9, 5), (0.1, 2.0 ** 301, 0.9, 0.9, 5)):
        with pytest.raises(ValueError):
            issref.iss(np.zeros((3, 3)), *bad)


def test_integer_bound_holds_for_a_full_row():
    """1024 points at the corners of the largest cube the radius admits around the first point's neighbourhood: |g| reaches 2^20 f and
    c S reaches its largest value; the assertions inside iss() are the check."""
    r = 1.0 - 2.0 ** -53    # f as close to 1 as a radius gets
    s = 0.57 * r            # half the cube's edge: the corners are 0.987 r from the centre
    corners = np.array([[a, b, c] for a in (-s, s) for b in (-s, s) for c in (-s, s)])
    p = np.concatenate([np.zeros((1, 3)), np.repeat(corners, 128, axis=0)[:1023]])
    got = issref.iss(p, r, r)
    assert got["cnt_salient"][0] == 1024 and issref.q_exponent(r) == 20
    g = int(np.floor(s * 2.0 ** 20))
    assert 1024 * 1023 * g * g > 2 ** 58   # the row is within a factor of 8 of the proven bound 2^61 on c S


def textbook(p, radius):
    """(c (n,), eigenvalues (n, 3) descending) of the covariance of { j : |p_j - p_i| < radius } in extended precision"""
    P = p.astype(LD)
    eig, cnt = np.zeros((len(p), 3)), np.zeros(len(p), dtype=np.int64)
    near = np.sqrt(knnref.dist2_matrix(p, p)) < radius
    for i in range(len(p)):
        nb = P[near[i]] - P[i]
        d = nb - nb.mean(0)
        cov = (d[:, :, None] * d[:, None, :]).sum(0) / LD(len(nb))
        eig[i] = np.linalg.eigvalsh(cov.astype(np.float64))[::-1]
        cnt[i] = len(nb)
    return cnt, eig


@pytest.mark.parametrize("name", ["bump", "bump_tight"])
def test_contract_is_iss(name):
    assert np.finfo(LD).eps < 1e-18, "needs an extended-precision long double"
    p, (rs, rn, g21, g32, mn) = issref.case(name)
    ref = issref.reference(name)
    cnt, eig = textbook(p, rs)
    assert (cnt == ref["cnt_salient"]).all()
    mine = ref["eig"] * 2.0 ** (-2 * ref["q"])
    err = np.abs(mine - eig).max(1) / eig[:, 0]
    print("largest eigenvalue error / l1:", err.max())
    assert err.max() < 1e-5
    want = (cnt >= mn) & (eig[:, 1] < g21 * eig[:, 0]) & (eig[:, 2] < g32 * eig[:, 1]) & (eig[:, 2] > 0)
    with np.errstate(all="ignore"):
        aside = (np.abs(eig[:, 1] / eig[:, 0] - g21) < 1e-3) | (np.abs(eig[:, 2] / eig[:, 1] - g32) < 1e-3)
    print("set aside:", int(aside.sum()), "of", len(p))
    assert aside.sum() <= 0.02 * len(p)
    assert (want[~aside] == ref["salient"][~aside]).all()
    assert ((ref["saliency"] > 0) == ref["salient"]).all()
    assert ref["salient"].any() and not ref["salient"].all()


def classes(name):
    """how many points of a case leave at each step of the definition"""
    (_, (rs, rn, g21, g32, mn)), r = issref.case(name), issref.reference(name)
    e, cs, cn, sal = r["eig"], r["cnt_salient"], r["cnt_nms"], r["saliency"]
    few = cs < mn
    f21 = ~few & ~(e[:, 1] < g21 * e[:, 0])
    f32 = ~few & ~f21 & ~(e[:, 2] < g32 * e[:, 1])
    few_nms = (sal > 0) & (cn < mn)
    beaten = (sal > 0) & ~few_nms & r["beaten"]
    return {"few": int(few.sum()), "gamma21": int(f21.sum()), "gamma32": int(f32.sum()), "few_nms": int(few_nms.sum()), "beaten": int(beaten.sum()),
            "keypoints": len(r["idx"]), "flat": int((e[:, 2] <= 0).sum()), "tied": int(r["tied"].sum())}


def test_cases_contain_what_they_are_for():
    """Measured: bump_tight 43 / 652 / 71 / 663 / 59 and 12 keypoints; the sheet has 60 points with l3 <= 0; every salient point of the
    duplicated cloud ties (1394 points); 295 points of the brick lattice tie with a neighbour.  The largest c_i is 104 (duplicates)."""
    got = classes("bump_tight")
    print(got)
    assert min(got[k] for k in ("few", "gamma21", "gamma32", "few_nms", "beaten")) >= 20 and got["keypoints"] > 0
    assert classes("sheet")["flat"] > 20
    p, _ = issref.case("duplicates")
    r = issref.reference("duplicates")
    assert (p[:700] == p[700:][np.argsort(np.random.Generator(np.random.PCG64(5)).permutation(700))]).all()
    assert (r["saliency"] > 0).sum() > 100 and (r["tied"] == (r["saliency"] > 0)).all()
    first = {}   # the lowest index of every distinct point
    for i, row in enumerate(map(bytes, p)):
        first.setdefault(row, i)
    assert all(first[bytes(p[i])] == i for i in r["idx"]) and len(r["idx"]) > 20
    assert classes("brick")["tied"] > 100
    assert max(int(issref.reference(n)["cnt_salient"].max()) for n in issref.CASES) < issref.CAP


FIX_N, FIX_PARAMS, FIX_TAU, FIX_MIN_COUNT = 4000, (0.6, 0.25, 0.975, 0.975, 5), 3.0, 4
MEASURED_DEG, MEASURED_SPACINGS = 2.02, 6.65   # the worst view of the docstring below


def test_chain_on_keypoints_reaches_the_refinement_basin():
    """The four-view fixture at 4000 points per view, descriptors of the full clouds, keypoints at (0.6 radius, 0.25 radius, 0.975, 0.975,
    5), both sides of every edge reduced to their keypoints, tau = 3 spacings, min_count = 4.  Measured with issref, fpfhref and initref
    on the CPU: 242 / 242 / 247 / 231 keypoints (6 % of the points), pairs 103, 93, 62, 93, 75, 64, inliers 11, 4, 2, 6, 7, 4, one
    component (parents -1, 0, 1, 1); the composed poses are 0.28 deg / 1.10 spacings, 1.13 deg / 1.90 and 2.01 deg / 6.65 from the truth.
    (Mode "src" on the same keypoints: inliers 26, 8, 3, 21, 20, 23 and 0.16 deg / 0.74, 0.74 deg / 2.40, 1.40 deg / 3.64.)
    The bound is three times the worst measured view, and in any case 5 deg / 10 spacings -- a guess at the basin of the point-to-plane
    refinement that nothing measured backs; here the second limit is the one that binds."""
    import fpfhref
    cl = ir.fixture_clouds(FIX_N)
    desc = [fpfhref.fpfh(cl["xyz"][k], cl["nrm"][k], cl["radius"], ir.FIX_MAX_NN)["desc"] for k in range(4)]
    params = (FIX_PARAMS[0] * cl["radius"], FIX_PARAMS[1] * cl["radius"]) + FIX_PARAMS[2:]
    r = issref.chain(cl["xyz"], desc, ir.FIX_EDGES, params, "both", FIX_TAU * cl["spacing"], ir.FIX_H, [ir.fix_seed(i, j) for i, j in ir.FIX_EDGES],
                     ir.FIX_EDGE_SIM, FIX_MIN_COUNT)
    print("keypoints", [len(k) for k in r["keypoints"]], "inliers", [e["count"] for e in r["edges"]])
    assert r["tree"]["components"] == 1
    assert all(0.02 * FIX_N < len(k) < 0.15 * FIX_N for k in r["keypoints"])
    for k in range(1, 4):
        deg, dt = ir.pose_error(r["tree"]["poses"][k], cl["gt"][k])
        print("frame", k, "deg", deg, "spacings", dt / cl["spacing"])
        assert deg < min(5.0, 3.0 * MEASURED_DEG) and dt < min(10.0, 3.0 * MEASURED_SPACINGS) * cl["spacing"]


# ---- the entry points
def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mvicp_iss_keypoints", "mvicp_iss_fetch"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)


def test_argument_errors_need_no_gpu(engine_lib):
    iss, fetch = engine_lib.mvicp_iss_keypoints, engine_lib.mvicp_iss_fetch
    assert iss(None, 0, 0.1, 0.1, 0.975, 0.975, 5) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, None, None, 0, None, None, None) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0, 2.0 ** -301, 2.0 ** 301):
        assert iss(ctx, 0, bad, 0.1, 0.975, 0.975, 5) == ERR_ARG and b"salient_radius" in engine_lib.mvicp_last_error(), bad
        assert iss(ctx, 0, 0.1, bad, 0.975, 0.975, 5) == ERR_ARG and b"non_max_radius" in engine_lib.mvicp_last_error(), bad
    for bad in (float("nan"), float("inf"), 0.0, -0.5):
        assert iss(ctx, 0, 0.1, 0.1, bad, 0.975, 5) == ERR_ARG and b"gamma21" in engine_lib.mvicp_last_error(), bad
        assert iss(ctx, 0, 0.1, 0.1, 0.975, bad, 5) == ERR_ARG and b"gamma32" in engine_lib.mvicp_last_error(), bad
    for bad in (-1, 0, 1025, 1 << 20):
        assert iss(ctx, 0, 0.1, 0.1, 0.975, 0.975, bad) == ERR_ARG and b"min_neighbors" in engine_lib.mvicp_last_error(), bad
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range)
        assert iss(ctx, frame, 2.0 ** -300, 2.0 ** 300, 0.975, 0.975, 1024) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert fake.raw == bytes(1 << 16)
