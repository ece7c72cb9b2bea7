"""-m gpu: conditioning sweep of linearize_sym_kernel + reduce_expand_kernel (csrc/linearize_sym.hip) against the extended-precision reference
of tests/symref.py, by the bar of tests/test_gpu_lin_accuracy.py.

Per piece (the 10 upper 3x3 sub-blocks of H, the 4 three-vectors of g, the cost): max|got - xref| / max|xref| within the piece; where xref is
exactly zero, got must be exactly zero.  Bar: the error of symref.blocks_fp64 (the direct world-frame rows in plain fp64, serial sums) against
the same reference on the same piece of the same case, floored at 2^-52, times MARGIN = 32.  Robust on and off.  tests/test_sym_cpu.py
checks on the CPU that the reference's rows are the objective's and that the kernel's algebra equals them.

Routes: explicit lists (p from the stream, n_p gathered through `first`), strict-subset lists (a `first` that is not the identity),
searched identity lists (p and n_p from the shared sorted cloud), a three-frame graph (interleaved launch order, an empty edge), and a
re-evaluation after mvicp_recompute_normals on the source frame.  Every case prints its worst ratio; the table is in DESIGN.md section 7.1."""
import numpy as np
import pytest

import lincases
import mvicp
import symcases
import symref
from mvicp import synth
from mvicp.lib import METRIC_SYMMETRIC

pytestmark = pytest.mark.gpu

MARGIN = 32.0
_REF_CACHE = {}


def _engine(case):
    eng = mvicp.Engine(0)
    if case["chunk"]:
        eng.set_option("lin_chunk", case["chunk"])    # takes effect at set_graph
    eng.set_frames([case["dst"], case["src"]], [case["nor"], case["snor"]])
    eng.set_graph([1], [0])
    return eng


def _references(p, q, nq, npn, Ps, Pd, a, key=None):
    """{robust: (xref, yardstick's piece errors)}"""
    if key is not None and key in _REF_CACHE:
        return _REF_CACHE[key]
    out = {}
    for robust in (1, 0):
        ref = symref.edge_block(p, q, nq, npn, Ps, Pd, a, robust)
        out[robust] = (ref, symref.piece_errors(symref.unpack(symref.blocks_fp64(p, q, nq, npn, Ps, Pd, a, robust)), ref))
    if key is not None:
        _REF_CACHE[key] = out
    return out


def _judge(blk, ref, err_ref, label, robust, failures):
    assert np.all(np.isfinite(blk)), (label, robust)
    err = symref.piece_errors(symref.unpack(blk), ref)
    ratio, where = symref.worst_ratio(err, err_ref)
    print("SYM   %-36s robust=%d  fp64 H %.1e g %.1e cost %.1e | kernel H %.1e g %.1e cost %.1e | worst ratio %.2f at %s" % (
        label, robust, max(v for k, v in err_ref.items() if k[0] == "H"), max((v for k, v in err_ref.items() if k[0] == "g" and np.isfinite(v)), default=0.0),
        err_ref["cost"], max(v for k, v in err.items() if k[0] == "H"), max(v for k, v in err.items() if k[0] == "g"), err["cost"], ratio, where))
    if not ratio <= MARGIN:
        failures.append((label, robust, where, ratio, err[where], err_ref[where]))


def _sweep_one(eng, case, first, second, a, label, key=None):
    p, q, nq, npn = symcases.gathered(case, first, second)
    refs = _references(p, q, nq, npn, case["poses"][1], case["poses"][0], a, key)
    failures = []
    for robust in (1, 0):
        blk = eng.linearize_metric(case["poses"], METRIC_SYMMETRIC, robust)[0]
        _judge(blk, refs[robust][0], refs[robust][1], label, robust, failures)
    return failures


def _run_explicit(name, kw, seed, key=None):
    case = symcases.make_case(name, seed=seed, **kw)
    eng = _engine(case)
    try:
        eng.set_correspondences(0, case["first"], case["second"], case["a"])
        return _sweep_one(eng, case, case["first"], case["second"], case["a"], name, key)
    finally:
        eng.close()


@pytest.mark.parametrize("family", list(symcases.FAMILIES))
def test_symmetric_sweep_explicit_lists(family):
    """every member of the families t, W, unit, a, zero, angle at N = 2 001 with explicit correspondences and scale"""
    failures = []
    for i, kw in enumerate(symcases.FAMILIES[family]):
        failures += _run_explicit(symcases.case_name(family, kw), kw, seed=400 + 13 * i + len(family))
    assert not failures, failures


@pytest.mark.parametrize("kw", symcases.COUNTS, ids=lambda kw: "N%d@%d" % (kw["N"], kw["chunk"]))
def test_symmetric_sweep_counts(kw):
    """tail lane (N = 1), one pair (2), a chunk less one / exactly / plus one (511, 512, 513 @ 512), one partial (513 @ 4096), 40 and 5 partials.
    The same seed per N: the two chunk sizes of an N see the same case, and its references are computed once."""
    failures = _run_explicit(symcases.case_name("count", kw), kw, seed=500 + kw["N"] % 97, key=("count", kw["N"]))
    assert not failures, failures


@pytest.mark.parametrize("kw", symcases.SUBSETS, ids=lambda kw: "N%dofM%d" % (kw["N"], kw["M"]))
def test_symmetric_sweep_strict_subset_lists(kw):
    """clouds of M points, a sorted random N-subset as the list: n_p comes through a `first` that is not the identity, p from the stream"""
    case = symcases.make_case("subset", seed=600, **kw)
    assert len(case["src"]) == kw["M"] and len(case["first"]) == kw["N"] and not np.array_equal(case["first"], np.arange(kw["N"]))
    failures = _run_explicit(symcases.case_name("subset", kw), kw, seed=600)
    assert not failures, failures


@pytest.mark.parametrize("share", [1, 0], ids=["shared", "lin_share_p=0"])
@pytest.mark.parametrize("kw", symcases.SEARCHED, ids=lambda kw: "N%d" % kw["N"])
def test_symmetric_sweep_searched_identity_lists(kw, share):
    """through mvicp_correspond with a cutoff that accepts every query: the list is the identity, so p and n_p both come from the shared
    sorted source cloud; lists and scale are what the search returned.  With option lin_share_p = 0 the same identity list takes the other
    route: p from the stream's private copy, n_p gathered through a `first` that is the identity."""
    name = symcases.case_name("searched" if share else "searched, lin_share_p=0", kw)
    case = symcases.make_case(name, seed=700, **kw)
    eng = _engine(case)
    try:
        eng.set_option("lin_share_p", share)
        counts, weights = eng.correspond(case["search_poses"], [1, 0], 100 * lincases.NOISE)
        assert counts[0] == len(case["src"]), (counts, len(case["src"]))
        first, second, _ = eng.get_correspondences(0)
        assert np.array_equal(first, np.arange(len(case["src"])))
        failures = _sweep_one(eng, case, first, second, weights[0], name)
    finally:
        eng.close()
    assert not failures, failures


def _unit_rows(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_symmetric_three_frame_graph_with_shared_sources_an_empty_edge_and_a_subset():
    """Three frames of 1 001 points, edges 1->0, 1->2, 2->0, 0->1: two edges share source 1 (the interleaved launch order), edge 2->0 has an
    explicit list of length 0, edge 1->2 a strict subset, the others every point.  Every edge's block against symref; the empty edge's
    block is all zeros."""
    rng = np.random.default_rng(808)
    n = 1001
    base = rng.normal(0, lincases.SPREAD, (n, 3))
    gt = [np.eye(4)]
    for k in (1, 2):
        P = np.eye(4); P[:3, :3] = synth.so3_exp(rng.normal(0, 0.5, 3)); P[:3, 3] = rng.normal(0, 0.3, 3)
        gt.append(P)
    pts, perms = [], []
    for k in range(3):
        perm = rng.permutation(n)
        Pinv = np.linalg.inv(gt[k])
        local = (base + rng.normal(0, lincases.NOISE, (n, 3))) @ Pinv[:3, :3].T + Pinv[:3, 3]
        c = np.empty_like(local); c[perm] = local       # point i of the base surface is stored at perm[i]
        pts.append(np.ascontiguousarray(c)); perms.append(perm)
    nor = [_unit_rows(rng, n) for _ in range(3)]
    poses = np.array([synth.add_noise(P, 2e-3, 1e-3, rng) for P in gt])
    src, dst = [1, 1, 2, 0], [0, 2, 0, 1]
    inv = [np.argsort(p) for p in perms]                # stored index -> base index
    lists = []
    for e, (s, d) in enumerate(zip(src, dst)):
        if e == 2:
            f = np.zeros(0, dtype=np.int32)
        elif e == 1:
            f = np.sort(rng.choice(n, 600, replace=False)).astype(np.int32)
        else:
            f = np.arange(n, dtype=np.int32)
        lists.append((f, perms[d][inv[s][f]].astype(np.int32)))
    a = np.float32(lincases.NOISE)
    eng = mvicp.Engine(0)
    try:
        eng.set_option("lin_chunk", 512)
        eng.set_frames(pts, nor)
        eng.set_graph(src, dst)
        for e, (f, sec) in enumerate(lists):
            eng.set_correspondences(e, f, sec, a)
        failures = []
        for robust in (1, 0):
            blocks = eng.linearize_metric(poses, METRIC_SYMMETRIC, robust)
            for e, (s, d) in enumerate(zip(src, dst)):
                f, sec = lists[e]
                if len(f) == 0:
                    assert not np.any(blocks[e]), (e, blocks[e])
                    continue
                p, q, nq, npn = pts[s][f], pts[d][sec], nor[d][sec], nor[s][f]
                ref = symref.edge_block(p, q, nq, npn, poses[s], poses[d], a, robust)
                err_ref = symref.piece_errors(symref.unpack(symref.blocks_fp64(p, q, nq, npn, poses[s], poses[d], a, robust)), ref)
                _judge(blocks[e], ref, err_ref, "graph edge %d (%d->%d, %d)" % (e, s, d, len(f)), robust, failures)
    finally:
        eng.close()
    assert not failures, failures


def test_symmetric_evaluation_sees_recomputed_source_normals():
    """mvicp_recompute_normals on the SOURCE frame between two symmetric evaluations: the first equals symref with the uploaded source normals,
    the second with the normals the call returned (the kernel reads the frame's current sorted normals, nothing is baked into the stream)"""
    kw = dict(N=2001, M=3000, chunk=512)
    case = symcases.make_case("recompute", seed=900, **kw)
    eng = _engine(case)
    try:
        eng.set_correspondences(0, case["first"], case["second"], case["a"])
        failures = _sweep_one(eng, case, case["first"], case["second"], case["a"], "before recompute_normals")
        new = eng.recompute_normals(1, 10)
        assert new.shape == case["snor"].shape and not np.allclose(new, case["snor"])
        case2 = dict(case, snor=new)
        failures += _sweep_one(eng, case2, case["first"], case["second"], case["a"], "after recompute_normals(src)")
    finally:
        eng.close()
    assert not failures, failures


NO_ROTATIONS = {"reflection": lambda R: R @ np.diag([1.0, 1.0, -1.0]), "3R": lambda R: 3.0 * R, "0.3R": lambda R: 0.3 * R, "zero": lambda R: np.zeros((3, 3))}


@pytest.mark.parametrize("kind", list(NO_ROTATIONS))
def test_symmetric_destination_that_is_no_rotation_gets_the_transpose(kind):
    """A destination matrix whose determinant is outside (0.5, 2) — a reflection (-1), 3 R (27), 0.3 R (0.027), the zero matrix — takes the other
    branch of the relative transform (api.cpp fill_rel_sym): R_d^T in the place of the inverse.  The blocks mean nothing there, but they are
    finite and they ARE the kernel's formulation with that substitution: symref.centred_blocks (which writes R_d^T) in long double.  The direct
    world-frame rows are no reference for such a matrix, so the yardstick is the same formulation in plain fp64 with serial sums, x MARGIN.
    N = 513 at chunk 512: two partials, the second a single tail lane."""
    case = symcases.make_case("no rotation: " + kind, seed=1100, N=513, chunk=512)
    poses = case["poses"].copy()
    poses[0][:3, :3] = NO_ROTATIONS[kind](case["poses"][0][:3, :3])
    det = np.linalg.det(poses[0][:3, :3])
    assert not 0.5 < det < 2.0, det
    p, q, nq, npn = symcases.gathered(case)
    eng = _engine(case)
    failures = []
    try:
        eng.set_correspondences(0, case["first"], case["second"], case["a"])
        for robust in (1, 0):
            blk = eng.linearize_metric(poses, METRIC_SYMMETRIC, robust)[0]
            ref = symref.centred_blocks(p, q, nq, npn, poses[1], poses[0], case["a"], robust)
            err_ref = symref.piece_errors(symref.centred_blocks(p, q, nq, npn, poses[1], poses[0], case["a"], robust, ftype=np.float64), ref)
            _judge(blk, ref, err_ref, "no rotation: %s (det %.3g)" % (kind, det), robust, failures)
    finally:
        eng.close()
    assert not failures, failures
