"""-m gpu: conditioning sweep of linearize_gicp_kernel + reduce_expand_kernel (csrc/linearize_gicp.hip) against the extended-precision reference
of tests/gicpref.py, by the bar and the piece definition of tests/test_gpu_sym_accuracy.py.

Per piece (the 10 upper 3x3 sub-blocks of H, the 4 three-vectors of g, the cost): max|got - xref| / max|xref| within the piece; where xref is
exactly zero, got must be exactly zero.  Bar: the error of gicpref.blocks_fp64 (the direct rows in plain fp64, serial sums) against the same
reference on the same piece of the same case, floored at 2^-52, times MARGIN = 32.  Robust on and off; epsilon 1e-3 and 1 everywhere, 1e-4 on
the angle family.  tests/test_gicp_cpu.py checks on the CPU that the reference's rows are the objective's.

Routes, at the sizes of the symmetric sweep (tests/symcases.py): explicit lists, a strict-subset list (a `first` that is not the identity), a
searched identity list with lin_share_p 1 and 0, a three-frame graph (interleaved launch order, an empty edge, a subset), and zero normals on
either side.  Normal families (tests/gicpcases.py), each on an explicit list of 2 001 of 3 000 at chunk 512 and on a searched identity list of
513: nearly parallel and antiparallel normals at epsilon 1e-6 ... 1, flipped normals (same bytes), normals of any length, and normals whose
n . n is subnormal, overflows, underflows or is not finite (the bytes of the case with those normals set to 0).  Every case prints its worst
ratio; the tables are in DESIGN.md section 3.17."""
import numpy as np
import pytest

import gicpcases
import gicpref
import lincases
import mvicp
import symcases
from mvicp import synth

pytestmark = pytest.mark.gpu

MARGIN = 32.0
EPSILONS = (1e-3, 1.0)
_REF_CACHE = {}


def _engine(case):
    eng = mvicp.Engine(0)
    if case["chunk"]:
        eng.set_option("lin_chunk", case["chunk"])    # takes effect at set_graph
    eng.set_frames([case["dst"], case["src"]], [case["nor"], case["snor"]])
    eng.set_graph([1], [0])
    return eng


def _references(p, q, nq, npn, Ps, Pd, a, eps, key=None):
    """{robust: (xref, yardstick's piece errors)}"""
    if key is not None and (key, eps) in _REF_CACHE:
        return _REF_CACHE[(key, eps)]
    out = {}
    for robust in (1, 0):
        ref = gicpref.edge_block(p, q, nq, npn, Ps, Pd, a, eps, robust)
        out[robust] = (ref, gicpref.piece_errors(gicpref.unpack(gicpref.blocks_fp64(p, q, nq, npn, Ps, Pd, a, eps, robust)), ref))
    if key is not None:
        _REF_CACHE[(key, eps)] = out
    return out


def _judge(blk, ref, err_ref, label, eps, robust, failures):
    assert np.all(np.isfinite(blk)), (label, eps, robust)
    err = gicpref.piece_errors(gicpref.unpack(blk), ref)
    ratio, where = gicpref.worst_ratio(err, err_ref)
    print("GICP  %-36s eps=%-6g robust=%d  fp64 H %.1e g %.1e cost %.1e | kernel H %.1e g %.1e cost %.1e | worst ratio %.2f at %s" % (
        label, eps, robust, max(v for k, v in err_ref.items() if k[0] == "H"), max((v for k, v in err_ref.items() if k[0] == "g" and np.isfinite(v)), default=0.0),
        err_ref["cost"], max(v for k, v in err.items() if k[0] == "H"), max(v for k, v in err.items() if k[0] == "g"), err["cost"], ratio, where))
    if not ratio <= MARGIN:
        failures.append((label, eps, robust, where, ratio, err[where], err_ref[where]))


def _sweep_one(eng, case, first, second, a, label, key=None, epsilons=EPSILONS):
    p, q, nq, npn = symcases.gathered(case, first, second)
    failures = []
    for eps in epsilons:
        refs = _references(p, q, nq, npn, case["poses"][1], case["poses"][0], a, eps, key)
        for robust in (1, 0):
            blk = eng.linearize_gicp(case["poses"], eps, robust)[0]
            _judge(blk, refs[robust][0], refs[robust][1], label, eps, robust, failures)
    return failures


def _run_explicit(name, kw, seed, key=None, epsilons=EPSILONS, edit=None):
    case = symcases.make_case(name, seed=seed, **kw)
    if edit is not None:
        edit(case)
    eng = _engine(case)
    try:
        eng.set_correspondences(0, case["first"], case["second"], case["a"])
        return _sweep_one(eng, case, case["first"], case["second"], case["a"], name, key, epsilons)
    finally:
        eng.close()


@pytest.mark.parametrize("family", list(symcases.FAMILIES))
def test_gicp_sweep_explicit_lists(family):
    """every member of the families t, W, unit, a, zero, angle at N = 2 001 with explicit correspondences and scale; the angle family also at
    epsilon = 1e-4"""
    failures = []
    eps = EPSILONS + ((1e-4,) if family == "angle" else ())
    for i, kw in enumerate(symcases.FAMILIES[family]):
        failures += _run_explicit(symcases.case_name(family, kw), kw, seed=400 + 13 * i + len(family), epsilons=eps)
    assert not failures, failures


@pytest.mark.parametrize("kw", symcases.COUNTS, ids=lambda kw: "N%d@%d" % (kw["N"], kw["chunk"]))
def test_gicp_sweep_counts(kw):
    """tail lane (N = 1), one pair (2), a chunk less one / exactly / plus one (511, 512, 513 @ 512), one partial (513 @ 4096), 40 and 5 partials.
    The same seed per N: the two chunk sizes of an N see the same case, and its references are computed once."""
    failures = _run_explicit(symcases.case_name("count", kw), kw, seed=500 + kw["N"] % 97, key=("count", kw["N"]))
    assert not failures, failures


def test_gicp_sweep_strict_subset_list():
    """clouds of 1 500 points, a sorted random 513-subset as the list: n_p comes through a `first` that is not the identity, p from the stream"""
    kw = symcases.SUBSETS[0]
    case = symcases.make_case("subset", seed=600, **kw)
    assert len(case["src"]) == kw["M"] and len(case["first"]) == kw["N"] and not np.array_equal(case["first"], np.arange(kw["N"]))
    failures = _run_explicit(symcases.case_name("subset", kw), kw, seed=600)
    assert not failures, failures


@pytest.mark.parametrize("share", [1, 0], ids=["shared", "lin_share_p=0"])
def test_gicp_sweep_searched_identity_list(share):
    """through mvicp_correspond with a cutoff that accepts every query: the list is the identity, so p and n_p both come from the shared sorted
    source cloud; with option lin_share_p = 0 the same list takes the other route (p from the stream, n_p through an identity `first`)."""
    kw = symcases.SEARCHED[0]
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


def test_gicp_three_frame_graph_with_shared_sources_an_empty_edge_and_a_subset():
    """Three frames of 1 001 points, edges 1->0, 1->2, 2->0, 0->1: two edges share source 1 (the interleaved launch order), edge 2->0 has an
    explicit list of length 0, edge 1->2 a strict subset, the others every point.  Every edge's block against gicpref; the empty edge's block
    is all zeros.  (The construction is that of the symmetric sweep's graph test.)"""
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
        for eps in EPSILONS:
            for robust in (1, 0):
                blocks = eng.linearize_gicp(poses, eps, robust)
                for e, (s, d) in enumerate(zip(src, dst)):
                    f, sec = lists[e]
                    if len(f) == 0:
                        assert not np.any(blocks[e]), (e, blocks[e])
                        continue
                    p, q, nq, npn = pts[s][f], pts[d][sec], nor[d][sec], nor[s][f]
                    ref = gicpref.edge_block(p, q, nq, npn, poses[s], poses[d], a, eps, robust)
                    err_ref = gicpref.piece_errors(gicpref.unpack(gicpref.blocks_fp64(p, q, nq, npn, poses[s], poses[d], a, eps, robust)), ref)
                    _judge(blocks[e], ref, err_ref, "graph edge %d (%d->%d, %d)" % (e, s, d, len(f)), eps, robust, failures)
    finally:
        eng.close()
    assert not failures, failures


def test_gicp_zero_normals_on_either_side():
    """n_q = 0 on some points of the destination, n_p = 0 on some of the source, both on a few pairs: C = I on that side (P(0) = 0), the block is
    finite and is gicpref's.  N = 2 001 of M = 3 000 at chunk 512: four partials, a gathered source normal."""
    def edit(case):
        rng = np.random.default_rng(77)
        case["nor"][rng.choice(len(case["nor"]), 700, replace=False)] = 0.0
        case["snor"][rng.choice(len(case["snor"]), 700, replace=False)] = 0.0
        p, q, nq, npn = symcases.gathered(case)
        zq, zp = ~np.any(nq != 0, axis=1), ~np.any(npn != 0, axis=1)
        assert (zq & ~zp).sum() > 100 and (zp & ~zq).sum() > 100 and (zp & zq).sum() > 10
    failures = _run_explicit("zero normals", dict(N=2001, M=3000, chunk=512), seed=1200, edit=edit)
    assert not failures, failures


# ---------------------------------------------------------------- normal families (tests/gicpcases.py)
# symcases draws n_q and n_p independently, so d = a^ . b^ is spread over [-1, 1] and Delta = 4 eps + c^2 |a^ x b^|^2 is seldom near its lower end.
# Each family below runs on two routes: an explicit list of 2 001 pairs on clouds of 3 000 at chunk 512 (four partials, an odd tail, n_p gathered
# through `first`), and a searched identity list of 513 at chunk 512 (the route of test_gicp_sweep_searched_identity_list).
FAMILY_ROUTES = {"explicit": dict(N=2001, M=3000, chunk=512), "searched": symcases.SEARCHED[0]}


def _family_blocks(route, seed, edit, epsilons, label, robusts=(1, 0)):
    """the case of `route` after edit(case) -> (case, first, second, a, {(eps, robust): block})"""
    case = symcases.make_case(label, seed=seed, **FAMILY_ROUTES[route])
    edit(case)
    eng = _engine(case)
    try:
        if route == "explicit":
            first, second, a = case["first"], case["second"], case["a"]
            eng.set_correspondences(0, first, second, a)
        else:
            counts, weights = eng.correspond(case["search_poses"], [1, 0], 100 * lincases.NOISE)
            assert counts[0] == len(case["src"]), (counts, len(case["src"]))
            first, second, _ = eng.get_correspondences(0)
            assert np.array_equal(first, np.arange(len(case["src"])))
            a = weights[0]
        blocks = {(eps, r): eng.linearize_gicp(case["poses"], eps, r)[0] for eps in epsilons for r in robusts}
    finally:
        eng.close()
    return case, first, second, a, blocks


def _judge_blocks(blocks, ref_case, first, second, a, label, failures):
    """every block against gicpref on the normals of ref_case, by the bar"""
    p, q, nq, npn = symcases.gathered(ref_case, first, second)
    for eps in sorted({k[0] for k in blocks}):
        refs = _references(p, q, nq, npn, ref_case["poses"][1], ref_case["poses"][0], a, eps)
        for (e, r), blk in blocks.items():
            if e == eps:
                _judge(blk, refs[r][0], refs[r][1], label, eps, r, failures)


@pytest.mark.parametrize("route", list(FAMILY_ROUTES))
@pytest.mark.parametrize("theta", gicpcases.THETAS, ids=gicpcases.theta_name)
def test_gicp_parallel_normals(theta, route):
    """n_p = A^T R(theta) n_q (gicpcases.parallel): theta = 0, 1e-8, 1e-4, 1e-2, pi - 1e-4, pi; epsilon = 1e-6, 1e-4, 1e-3, 1; robust on and off.  The
    normals of a registration: Delta = 4 eps + c^2 |a^ x b^|^2 at its lower end, kappa = eps c / Delta at its largest — the regime of the claim
    that nothing cancels as the normals become parallel (csrc/linearize_gicp.hip), which tests/test_gicp_cpu.py checks for the reference only.
    The reference at epsilon = 1e-6: gicpref's long-double W resolves 2^-64 / eps = 5e-14 there (5e-16 at 1e-4, gicpref's docstring), and the
    fp64 yardstick's worst piece is about 2e-10 (2e-12 at 1e-4, 2e-13 at 1e-3, 4e-14 at 1; CPU, N = 513), so the reference is far inside the bar.
    The bar at 1e-6 is LOOSE for the same reason: it catches a wrong limit, not a cancellation no worse than the cofactor inverse's — so every
    case prints the kernel's own error next to the yardstick's (the GICP lines; table in DESIGN.md section 3.17)."""
    label = "parallel theta=%s %s" % (gicpcases.theta_name(theta), route)
    case, first, second, a, blocks = _family_blocks(route, 1300, lambda c: gicpcases.parallel(c, theta), gicpcases.PARALLEL_EPSILONS, label)
    p, q, nq, npn = symcases.gathered(case, first, second)
    A = case["poses"][0][:3, :3].T @ case["poses"][1][:3, :3]
    cosang = np.einsum("ij,ij->i", nq, npn @ A.T)
    assert np.median(np.abs(cosang - np.cos(theta))) <= 1e-12       # the list's pairs carry the tilt asked for
    failures = []
    _judge_blocks(blocks, case, first, second, a, label, failures)
    assert not failures, failures


@pytest.mark.parametrize("route", list(FAMILY_ROUTES))
def test_gicp_flipped_normals_give_the_same_bytes(route):
    """A random half of the destination normals and, independently, of the source normals negated: the blocks equal the unflipped case's byte for
    byte (epsilon 1e-3 and 1, robust on and off), and are gicpref's for the flipped normals by the bar.  By the operation order of
    csrc/linearize_gicp.hip: nu -> -nu and a^ -> -a^ exactly (every product changes sign, no sum is reordered); d and k2 change sign; a' changes
    sign with a^ (or b' with b^); z -> -z leaves |z|^2; so every W_ij = fma(b^_i, b'_j, fma(a^_i, a'_j, .)) is unchanged bit for bit."""
    label = "sign " + route
    _, _, _, _, plain = _family_blocks(route, 1400, lambda c: None, EPSILONS, label + " (unflipped)")
    case, first, second, a, blocks = _family_blocks(route, 1400, gicpcases.sign, EPSILONS, label)
    p, q, nq, npn = symcases.gathered(case, first, second)
    assert np.all(np.abs(np.linalg.norm(nq, axis=1) - 1) < 1e-12)
    failures = []
    _judge_blocks(blocks, case, first, second, a, label, failures)
    for k in blocks:
        assert blocks[k].tobytes() == plain[k].tobytes(), (route, k, float(np.abs(blocks[k] - plain[k]).max()))
    assert not failures, failures


@pytest.mark.parametrize("route", list(FAMILY_ROUTES))
def test_gicp_normals_of_any_length(route):
    """Every normal of both sides times 2^k, k uniform in [-500, 500] per normal: gicpref's by the bar (P(n) does not depend on |n|; n . n stays a
    normal number, where fast_rsqrt is used outside the range lin_common.h documents it for).  Printed, not asserted: whether the bytes are the
    unscaled case's (v_rsq_f64 and the Newton steps need not commute with a power of 4)."""
    label = "length " + route
    _, _, _, _, plain = _family_blocks(route, 1500, lambda c: None, EPSILONS, label + " (unscaled)")
    case, first, second, a, blocks = _family_blocks(route, 1500, gicpcases.length, EPSILONS, label)
    failures = []
    _judge_blocks(blocks, case, first, second, a, label, failures)
    print("GICP  %s: bytes equal to the unscaled case's: %s" % (label, {k: blocks[k].tobytes() == plain[k].tobytes() for k in blocks}))
    assert not failures, failures


def _as_missing(route, seed, family, label):
    """the rows family(case) spoils must count as missing normals: finite blocks, byte for byte those of the same case with these rows set to 0, and
    gicpref's for the zeroed normals by the bar"""
    rows = {}
    case, first, second, a, blocks = _family_blocks(route, seed, lambda c: rows.update(r=family(c)), EPSILONS, label)
    zcase = gicpcases.zeroed(case, rows["r"])

    def put_zeroed(c):
        c["nor"][:] = zcase["nor"]; c["snor"][:] = zcase["snor"]

    _, zfirst, zsecond, za, zblocks = _family_blocks(route, seed, put_zeroed, EPSILONS, label + " (zeroed)")
    assert np.array_equal(first, zfirst) and np.array_equal(second, zsecond) and a == za
    p, q, nq, npn = symcases.gathered(zcase, first, second)
    zq, zp = ~np.any(nq != 0, axis=1), ~np.any(npn != 0, axis=1)
    assert (zq & ~zp).sum() >= 100 and (zp & ~zq).sum() >= 100 and (zp & zq).sum() >= 4, ((zq & ~zp).sum(), (zp & ~zq).sum(), (zp & zq).sum())
    failures = []
    for k in blocks:
        assert np.all(np.isfinite(blocks[k])), (label, k)
    _judge_blocks(blocks, zcase, first, second, a, label, failures)
    for k in blocks:
        assert blocks[k].tobytes() == zblocks[k].tobytes(), (label, k, float(np.abs(blocks[k] - zblocks[k]).max()))
    assert not failures, failures


@pytest.mark.parametrize("route", list(FAMILY_ROUTES))
def test_gicp_subnormal_n_dot_n_is_a_missing_normal(route):
    """Rows scaled to lengths 2^-536 ... 2^-512: n . n is a subnormal fp64 number with 2 to 50 bits left.  With the predicate `n . n > 0` the kernel's a^
    was off unit length by up to 2^-2 there and the block missed gicpref by far more than any bar (tests/test_gicp_cpu.py shows it on the CPU).
    On an MI355X that build's pieces were off by up to 1.6 (H), 1.1 (g), 0.6 (cost) relative at epsilon = 1e-3 on these cases.
    The contract now asks 2^-1022 <= n . n < inf, taken on the fp64 value, and these rows count as missing normals."""
    _as_missing(route, 1600, gicpcases.subnormal, "subnormal " + route)


@pytest.mark.parametrize("route", list(FAMILY_ROUTES))
def test_gicp_nonfinite_and_out_of_range_normals_are_missing_normals(route):
    """A NaN component, a +-Inf component, components of 1e200 (n . n overflows), components of 1e-200 (n . n underflows to 0), on about 300 rows of
    each side and on both sides of a few pairs.  mvicp_set_frame does not look at normals, so all of them reach the kernel."""
    _as_missing(route, 1700, gicpcases.nonfinite, "nonfinite " + route)
