"""The contract of mvicp_boundary on the CPU: tests/boundref.py's numpy form equals its scalar loop on every cloud the GPU tests use; the flat
lattice gives the pinned patterns; the end-to-end clouds give the recorded counts, and negated normals the same flags; a planted hole is
found and nothing far from an edge is flagged; rejecting pairs on the target's boundary points brings the registration of the partial pair
closer to the truth; mvicp.reject_by_mask; the symbols exist and the argument errors need no GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import boundref as br
from boundref import reference
import matchref
import mvicp
import symref
import test_sym_cpu
from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("mvicp_boundary", "mvicp_boundary_fetch", "mvicp_boundary_select", "mvicp_boundary_fetch_kept")
LOOP_ROWS = 400   # the scalar loop runs over the first rows of a large cloud only (a row is independent of the others)


def _all_runs():
    return [(name, r) for name, (_, _, runs) in sorted(br.cases().items()) for r in range(len(runs))]


@pytest.mark.parametrize("name,run", _all_runs())
def test_numpy_form_equals_the_scalar_loop(name, run):
    p, N, runs = br.cases()[name]
    got = reference(name, run)
    m = min(len(p), LOOP_ROWS)
    want = br.boundary_loop(p, N, *runs[run], rows=got["knn"], points=range(m))
    for key, dt in br.KEYS:
        assert got[key].dtype == dt and got[key][:m].tobytes() == want[key][:m].tobytes(), (name, runs[run], key)
    assert got["boundary"] == int(got["flag"].sum()) and ((got["open"] > 0) == (got["flag"] == 1)).all()
    assert (got["valid"] <= got["used"]).all() and (got["open"] <= got["valid"]).all()
    for boundary in (True, False):
        sel = br.select(p, N, got, boundary)
        assert (np.diff(sel["idx"]) > 0).all() and sel["xyz"].tobytes() == p[sel["idx"]].tobytes() and sel["nrm"].tobytes() == N[sel["idx"]].tobytes()
    assert br.select(p, N, got, True)["kept"] + br.select(p, None, got, False)["kept"] == len(p)


def test_the_cases_hold_what_they_are_for():
    """The facts the GPU tests rely on, on the reference alone: every case but the degenerate ones holds flagged and unflagged points, and
    undecided ones where it is there for them.  No case can pass by flagging nothing."""
    R = lambda name, run: reference(name, run)
    # three entries = two directions: one of the two gaps is at least 180 degrees, so every point is flagged; the rest hold both kinds
    assert R("blob", 0)["boundary"] == 2000 and (R("blob", 0)["valid"] == 2).all()
    for run in (1, 2):
        assert 30 < R("blob", run)["boundary"] < 1000
    assert (R("e2e dst", 0)["boundary"], R("e2e dst", 1)["boundary"]) == (130, 184)
    k5, k9 = R("lattice, shuffled", 0), R("lattice, shuffled", 1)
    # (the shuffle changes the tie order of the rows, and with it the corners: the interior stays 4, the border 2 or 1)
    assert (k5["open"] == 4).sum() == 25 and set(k5["open"][k5["open"] != 4].tolist()) == {1, 2} and k5["boundary"] == 49
    assert (k9["open"] == 0).sum() == 25 and k9["boundary"] == 24
    # rows of copies: no direction, nothing flagged, and that is not "undecided by the normal"; at 30 the row reaches other points
    for run in (0, 1):
        d = R("duplicated", run)
        assert (d["valid"] == 0).all() and d["boundary"] == 0 and (d["used"] == (5, 6)[run]).all()
    assert 0 < R("duplicated", 2)["boundary"] < 720 and (R("duplicated", 2)["valid"] == 24).all()
    for run in (0, 1):
        c = R("collinear", run)
        assert c["boundary"] == 300 and (c["valid"] == 7).all()
    nl = R("normal lengths", 0)
    assert (nl["valid"][2::4] == 0).all() and (nl["valid"][3::4] == 0).all() and not nl["flag"][2::4].any() and not nl["flag"][3::4].any()
    assert (nl["valid"][0::4] == 15).all() and (nl["valid"][1::4] == 15).all()
    for part in (nl["flag"][0::4], nl["flag"][1::4]):
        assert 0 < part.sum() < len(part)
    sc = R("scale 1e-3 at 1e3", 0)
    assert 0 < sc["boundary"] < 800 and (sc["valid"] >= 14).all()
    for run in (0, 1):
        h = R("hybrid rows", run)
        assert sorted(set(h["used"].tolist())) == list(range(1, 9)) and 0 < h["boundary"] < 800
        assert (h["valid"][h["used"] < 3] == 0).all() and (h["valid"][h["used"] >= 3] == h["used"][h["used"] >= 3] - 1).all()
    assert [R("n = %d" % m, 0)["boundary"] for m in (0, 1, 2, 3)] == [0, 0, 0, 3]


@pytest.mark.parametrize("k", [5, 9])
def test_the_flat_lattice_gives_the_pinned_pattern(k):
    """Neighbours exactly 90 degrees apart at cos_gap = 0: the dot product is exactly 0 and the strict inequality decides.  k = 5 (the point
    and its 4 axis neighbours): every interior direction looks into a gap of exactly 90 degrees, open = 4; edges 2; corners 2 or 1 as the
    row's tie order gives.  k = 9 (the diagonals too): neighbours 45 degrees apart, no interior gap."""
    p, N = br.lattice7()
    want = br.LATTICE_K5 if k == 5 else br.LATTICE_K9
    for f in (br.boundary, br.boundary_loop):
        got = f(p, N, k, 0.0, 0.0)
        assert (got["open"].reshape(7, 7) == want).all(), got["open"].reshape(7, 7)
        assert (got["flag"].reshape(7, 7) == (want > 0)).all() and (got["used"] == k).all()
    assert (want[1:6, 1:6] == (4 if k == 5 else 0)).all()


@pytest.mark.parametrize("partial", [False, True])
def test_the_end_to_end_clouds_give_the_recorded_counts(partial):
    cl = matchref.e2e_clouds(partial)
    for cos_gap, want in ((-0.5, (131, 131) if partial else (131, 130)), (0.0, (190, 178) if partial else (190, 184))):
        rs = br.boundary(cl["src"], cl["src_nrm"], 30, 0.0, cos_gap)
        rd = br.boundary(cl["dst"], cl["dst_nrm"], 30, 0.0, cos_gap)
        assert (rs["boundary"], rd["boundary"]) == want
        assert min(rs["valid"].min(), rd["valid"].min()) >= 29
        if cos_gap == -0.5:
            assert max(rs["open"].max(), rd["open"].max()) <= 1   # (two gaps of 120 degrees or more leave little room for 29 neighbours)
        # negating N mirrors the plane: the flags are promised equal up to rounding at the threshold, and on these clouds they are equal
        for c, N, r in ((cl["src"], cl["src_nrm"], rs), (cl["dst"], cl["dst_nrm"], rd)):
            assert (br.boundary(c, -N, 30, 0.0, cos_gap, rows=r["knn"])["flag"] == r["flag"]).all()


def test_a_planted_hole_is_found_and_the_interior_is_not_flagged():
    """A jittered 41 x 41 sheet (pitch 1, jitter +-0.2) with a circular hole of radius 6: 1 567 points.  Observed on the reference at (16,
    -0.5) and (30, -0.5): 196 flagged; all 21 points within half a spacing of the rim are flagged, 36 of the 41 within one; the flagged
    point farthest from the rim and from the outline is 0.97 spacings away.  Asserted: the rim points within half a spacing are flagged,
    and no point farther than HOLE_MARGIN = 1.5 spacings from both is (one pitch plus the jitter of 0.2 on either side)."""
    p, N, rim, outline = br.holed_sheet()
    assert len(p) == 1567
    near = np.minimum(rim, outline)
    for k in (16, 30):
        r = br.boundary(p, N, k, 0.0, -0.5)
        f = r["flag"] == 1
        print("k = %d: %d flagged, %d of %d within 0.5 of the rim, %d of %d within 1.0; the farthest flagged point is %.3f spacings from an edge" % (
            k, r["boundary"], f[rim < 0.5].sum(), (rim < 0.5).sum(), f[rim < 1.0].sum(), (rim < 1.0).sum(), near[f].max()))
        assert (rim < 0.5).sum() >= 20 and f[rim < 0.5].all()
        assert not f[near > br.HOLE_MARGIN].any() and (near > br.HOLE_MARGIN).sum() > 1000


def boundary_registration(cl, symmetric, dst_mask, cutoff_spacings=3.0, rounds=25):
    """test_sym_cpu.host_registration's loop with the pairs on flagged target points dropped between the search and the solve (the edge's
    scale stays as searched) -> final pose of src"""
    src, dst, sn, dn = cl["src"], cl["dst"], cl["src_nrm"], cl["dst_nrm"]
    P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
    for _ in range(rounds):
        first, second, a = symref.nn_cutoff(src, P[1], dst, P[0], cutoff_spacings * cl["spacing"])
        first, second = mvicp.reject_by_mask(first, second, None, dst_mask)
        p, q, nq, npn = src[first], dst[second], dn[second], sn[first]

        def evaluate(poses):
            if symmetric:
                return symref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], a, True)[None, :]
            return test_sym_cpu._plane_fp64(p, q, nq, poses[1], poses[0], a, True)[None, :]

        P, _ = L.lm_solve_host(2, [1], [0], P, [1, 0], L.PARAM_SOPHUS_SE3, evaluate, 50)
    return P[1]


@functools.lru_cache(maxsize=None)
def registration_figures(partial, symmetric):
    """-> ((deg, spacings) without rejection, (deg, spacings) with target-side rejection at (30, -0.5)); shared with the GPU test"""
    cl = matchref.e2e_clouds(partial)
    mask = br.boundary(cl["dst"], cl["dst_nrm"], 30, 0.0, -0.5)["flag"]
    none = symref.distance_to_truth(test_sym_cpu.host_registration(cl, symmetric), cl["truth"], cl["src"], cl["spacing"])
    rej = symref.distance_to_truth(boundary_registration(cl, symmetric, mask), cl["truth"], cl["src"], cl["spacing"])
    return none, rej


@pytest.mark.parametrize("symmetric", [False, True])
def test_target_side_rejection_ends_closer_to_the_truth_on_the_partial_pair(symmetric):
    """The behaviour the stage exists for.  A numpy prototype gave, without / with rejection: partial pair, point-to-plane 0.0817 deg /
    0.1091 spacings -> 0.0467 / 0.0716, symmetric 0.0041 / 0.0083 -> 0.0017 / 0.0032; full pair, point-to-plane 0.0315 / 0.0549 ->
    0.0306 / 0.0497, symmetric 0.0045 / 0.0063 -> 0.0043 / 0.0061.  Asserted: the ordering on the partial pair, in both measures.  The
    full pair is printed."""
    for partial in (True, False):
        none, rej = registration_figures(partial, symmetric)
        print("partial=%s symmetric=%s  none %.4f deg, %.4f spacings  |  target-side rejection %.4f deg, %.4f spacings" % (
            partial, symmetric, none[0], none[1], rej[0], rej[1]))
        if partial:
            assert rej[0] < none[0] and rej[1] < none[1], (none, rej)


def test_reject_by_mask():
    first = np.array([0, 1, 2, 3, 5], dtype=np.int32); second = np.array([4, 4, 0, 1, 2], dtype=np.int32)
    src = np.array([0, 1, 0, 0, 0, 0], dtype=np.uint8); dst = np.array([0, 1, 0, 0, 0], dtype=np.uint8)
    for sm, dm, keep in ((None, None, [0, 1, 2, 3, 4]), (src, None, [0, 2, 3, 4]), (None, dst, [0, 1, 2, 4]), (src, dst, [0, 2, 4]), (None, dst != 0, [0, 1, 2, 4])):
        f, s = mvicp.reject_by_mask(first, second, sm, dm)
        assert f.dtype == np.int32 and s.dtype == np.int32 and f.tolist() == first[keep].tolist() and s.tolist() == second[keep].tolist()
        rf, rs = br.reject_by_mask(first, second, sm, dm)
        assert f.tobytes() == rf.tobytes() and s.tobytes() == rs.tobytes()
    f, s = mvicp.reject_by_mask(first[:0], second[:0], src, dst)
    assert len(f) == 0 and len(s) == 0
    with pytest.raises(ValueError):
        mvicp.reject_by_mask(first, second[:3], None, None)


def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)
    for name in ("boundary", "boundary_select", "reject_correspondences"):
        assert hasattr(mvicp.Engine, name)
    assert hasattr(mvicp, "reject_by_mask")


def test_argument_errors_need_no_gpu(engine_lib):
    bnd, fetch, select, kept = engine_lib.mvicp_boundary, engine_lib.mvicp_boundary_fetch, engine_lib.mvicp_boundary_select, engine_lib.mvicp_boundary_fetch_kept
    assert bnd(None, 0, 0, 30, 0.0, -0.5) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, None, None, None) == ERR_ARG and select(None, 1) == ERR_ARG and kept(None, 0, None, None, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for source in (-1, 2):
        assert bnd(ctx, 0, source, 30, 0.0, -0.5) == ERR_ARG and b"source" in engine_lib.mvicp_last_error(), source
    for k in (2, 65, 0, -1):
        assert bnd(ctx, 0, 0, k, 0.0, -0.5) == ERR_ARG and b"max_nn" in engine_lib.mvicp_last_error(), k
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert bnd(ctx, 0, 0, 30, bad, -0.5) == ERR_ARG and b"radius" in engine_lib.mvicp_last_error(), bad
    for bad in (-1.0, 1.0, 1.5, -2.0, float("nan"), float("inf"), -float("inf")):
        assert bnd(ctx, 0, 0, 30, 0.0, bad) == ERR_ARG and b"cos_gap" in engine_lib.mvicp_last_error(), bad
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range)
        assert bnd(ctx, frame, 0, 30, 0.0, -0.5) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert fake.raw == bytes(1 << 16)


def test_without_a_gpu_the_call_fails_loudly(engine_lib):
    """No device, no context, no boundary: mvicp_create refuses (there is no CPU path) and mvicp_boundary on the context it did not make
    reports an error instead of an answer.  With a device the same calls succeed on an empty context."""
    h = C.c_void_p()
    st = engine_lib.mvicp_create(0, C.byref(h))
    try:
        if st != 0:
            assert st == -2 and not h.value and b"no CPU fallback" in engine_lib.mvicp_last_error()
            with pytest.raises(mvicp.MvicpError):
                mvicp.Engine(0)
        assert engine_lib.mvicp_boundary(h, 0, 0, 30, 0.0, -0.5) == ERR_ARG   # a NULL context, or a context without frames
        assert len(engine_lib.mvicp_last_error()) > 0
    finally:
        if h.value:
            engine_lib.mvicp_destroy(h)
