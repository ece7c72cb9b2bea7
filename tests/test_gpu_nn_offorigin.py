"""Nearest-neighbour search away from the origin: every NN kernel and every kind of cached round against the oracle on problems that
tests/offorigin.py has placed at a local site frame, at 1e6 m, and at UTM coordinates (metres and millimetres).

What scales with absolute coordinates in the kernels: the fp32 boxes and the patch-box slack, the matrix-pipe kernel's block-local f16
operands and -T pieces, the hash cell assignment and its clamp, and the rounding allowance of the temporal cache."""
import numpy as np
import pytest

import depthcases as dc
import mvicp
import offorigin as oo
from mvicp import lib as L
from mvicp import synth
from test_gpu_parity import TREE, _Eng, _random_cloud

pytestmark = pytest.mark.gpu

QUERY_METHODS = [("brute", L.NN_BRUTE, None), ("grid", L.NN_GRID, None), ("tree", TREE, None), ("tile0", L.NN_TILE, 0), ("tile2", L.NN_TILE, 2)]


@pytest.fixture(scope="module")
def eng():
    e = _Eng(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def edge_eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


# the one-edge route at depths 1 and 2: (launch string of a 2-level target, of a 1-level target), from the table of tests/depthcases.py
EDGE_BUILDS = [(k, "%s<%d,-1,%s" % (dc.parse_launch(k)["kernel"], dc.parse_launch(k)["WPE"], k.split(",", 2)[2])) for k, _ in dc.variants(2)]


def _edge_all(e, orc, dst, q, ri, od, tag):
    """The same query set as the source cloud of one edge (identity poses, a cutoff above every distance): nn_tile_kernel and
    nn_mfma_kernel themselves, in the build of the target's depth (asserted through Engine.last_nn_launch)."""
    thresh = dc.cutoff_above(od)
    expected = dc.expected_list(orc, ri, od, thresh)
    frames, src, dsts, poses, fixed = dc.edge_frames([dst], q)
    e.set_frames(frames, None); e.set_graph(src, dsts)
    depth = int(e.get_structure(0, "scalars")[13])
    assert depth == dc.levels(len(dst)) and depth in (1, 2), (tag, depth)
    for two, one in EDGE_BUILDS:
        want = two if depth == 2 else one
        launch = None
        for r, c, w, launch in dc.search_variant(e, dc.VARIANTS[two], poses, fixed, thresh):
            gf, gs, gd = e.get_correspondences(0)
            bad = np.nonzero((gs != expected[1]) | (gd != expected[2]))[0] if len(gs) == len(expected[1]) else np.array([-1])
            assert c[0] == len(q) and np.array_equal(gf, expected[0]) and len(bad) == 0, (tag, want, r, launch, len(bad), bad[:5].tolist())
            assert w[0] == expected[3], (tag, want, r)
        assert launch == want, (tag, want, launch)


def _query_all(eng, orc, refnn, dst, q, tag, methods=QUERY_METHODS, edge_eng=None):
    """Distances: the oracle's brute force.  Indices: the real nanoflann's, which is the oracle's lowest index except where the best
    distance is met by several targets (a query 1e6 m from a millimetre cloud ties with half of it): there the reference keeps the
    target its tree visits first, and so must every kernel (test_duplicate_targets_follow_nanoflanns_visit_order)."""
    eng.set_frames([dst], None)
    oi, od = orc.nn_brute(dst, q)
    ri, rd = refnn.query(dst, q)
    assert np.array_equal(rd, od), tag
    for name, m, mfma in methods:
        if mfma is not None:
            eng.set_option("tile_mfma", mfma)
        idx, d2 = eng.nn_query(0, q, m)
        bad = np.nonzero((idx != ri) | (d2 != od))[0]
        assert len(bad) == 0, (tag, name, len(bad), bad[:5].tolist(), idx[bad[:5]].tolist(), ri[bad[:5]].tolist(), oi[bad[:5]].tolist())
    if edge_eng is not None:
        _edge_all(edge_eng, orc, dst, q, ri, od, tag)


# ---------------------------------------------------------------- a. single queries
@pytest.mark.parametrize("kind", ["blob", "plane", "lattice", "clusters"])
@pytest.mark.parametrize("place", ["unit", "local", "mm_local", "local1e6"])
def test_single_queries_every_kernel(eng, edge_eng, orc, refnn, place, kind):
    """nn_query through brute force, hash grid and tree only, clouds of 1 .. 3000 points: queries = another cloud's points, the target's
    own points +- 1e-9 of the data scale, a blob, and two far ones (1e3 extents and 1e6 m away).  The rows `tile0` and `tile2` of nn_query
    are the GRID kernel three times over (mvicp_nn_query maps NN_TILE and NN_AUTO to it: raw queries are not patch-ordered); they stay as
    rows of that entry point.  The two tile kernels see the same query sets as the source cloud of one edge (_edge_all): 1 .. 777 points
    are 1-level targets (the generic builds), 3000 points a 2-level one (the <.., 1, ..> builds), unseeded, seeded and counting."""
    assert refnn is not None, "oracle/_ref (real nanoflann) was not built"
    rng = np.random.default_rng(sum(map(ord, place + kind)))
    s = oo.place_scale(place)
    others = {"blob": "plane", "plane": "clusters", "lattice": "blob", "clusters": "lattice"}
    try:
        for n in (1, 65, 777, 3000):
            dst = oo.place_points(place, _random_cloud(rng, n, kind, 1.0))
            other = oo.place_points(place, _random_cloud(rng, 500, others[kind], 1.0))
            near = dst[: min(n, 400)] + rng.choice([-1e-9, 1e-9], (min(n, 400), 3)) * s
            blob = oo.place_points(place, _random_cloud(rng, 100, "blob", 1.0))
            centre = dst.mean(0)
            extent = max(float(np.ptp(dst, axis=0).max()), s)
            far = np.array([centre + 1e3 * extent * np.array([0.6, -0.64, 0.48]), centre + np.array([0.0, 0.0, 1e6])])
            _query_all(eng, orc, refnn, dst, np.ascontiguousarray(np.vstack([other, near, blob, far])), (place, kind, n), edge_eng=edge_eng)
    finally:
        eng.set_option("tile_mfma", 1)   # the default


# ---------------------------------------------------------------- b. deep density contrast
def test_deep_density_contrast_at_a_local_site_frame(eng, orc, refnn):
    """2000 points within a micrometre of one spot, 500 over a kilometre, a 700-point line — all 850 m from the origin: the hash block
    test must hand over to the tree exactly when it cannot prove optimality, and the tree's fp32 boxes must stay outward."""
    assert refnn is not None, "oracle/_ref (real nanoflann) was not built"
    rng = np.random.default_rng(21)
    spot = np.array([3.0, -2.0, 1.0])
    a = spot + rng.uniform(-1e-6, 1e-6, (2000, 3))
    b = rng.uniform(-500.0, 500.0, (500, 3))
    c = np.stack([np.linspace(-400, 400, 700), np.full(700, 7.0), np.full(700, -3.0)], 1)
    dst = oo.place_points("local", np.vstack([a, b, c]))
    q = np.vstack([spot + rng.normal(0, 2e-6, (1500, 3)), spot + rng.normal(0, 1e-3, (500, 3)), rng.uniform(-600, 600, (1500, 3)),
                   a[::5] + 1e-9, [[100.0, -50.0, 1e6]], [[1e6, 0.0, 0.0]]])
    q = oo.place_points("local", q)
    _query_all(eng, orc, refnn, dst, q, "deep", [("grid", L.NN_GRID, None), ("tree", TREE, None)])


# ---------------------------------------------------------------- c. rounds
MAGS = [3e-3, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7]
ROUND_METHODS = {"grid": (L.NN_GRID, {}), "tile0": (L.NN_TILE, {"tile_mfma": 0, "tile_bounds": 2}),
                 "tile2": (L.NN_TILE, {"tile_mfma": 2, "tile_bounds": 2}), "auto": (L.NN_AUTO, {})}
ORACLE_ROUNDS = (1, len(MAGS))        # the first and the last moving round (the repeated round has the last one's inputs)
_PLACED = {}


def _placed_rounds(orc, place):
    """The placed problem, its scripted pose sequence and the oracle's lists of the compared rounds: computed once per placement."""
    if place not in _PLACED:
        pb = synth.make_problem(4, 3000 if place == "local1e6" else 6000)
        seq = oo.scripted_poses(pb["init"], MAGS, 11)
        pts, nor, _, thresh, pl = oo.place(place, pb["pts"], pb["nor"], seq[0], 0.05)
        poses = [pl.poses(P) for P in seq]
        ref = {}
        for r in ORACLE_ROUNDS:
            ref[r] = [orc.correspond_edge(pts[s], poses[r][s], pts[d], poses[r][d], thresh) for s, d in zip(pb["src"], pb["dst"])]
        ref[len(MAGS) + 1] = ref[len(MAGS)]
        _PLACED[place] = (pb, pts, nor, poses, thresh, ref)
    return _PLACED[place]


@pytest.mark.parametrize("method", list(ROUND_METHODS))
@pytest.mark.parametrize("place", list(oo.PLACEMENTS))
def test_cached_rounds_equal_the_uncached_twin_and_the_oracle(orc, place, method):
    """A search, six rounds of shrinking scripted moves (3e-3 .. 1e-7) and the last poses once more, beside a twin engine without the
    temporal cache and without list reuse: counts, float weights and the three list arrays are the twin's after every round and the
    oracle's after the first moving, the last moving and the repeated round.  On the grid kernel the cache must really engage in the
    1e-7 round (hit fraction > 0.5, the bar of test_tile_kernel_lower_bounds_feed_the_temporal_cache for this problem and this move): a
    rigorous allowance at 4e6 m is ~3e-9 m, far below the guard band (2e-4 m, 2e-7 m for millimetre data), so exactness cannot cost these hits.  `utm_apart` is exempt:
    four of its six edges have no neighbour within the search radius at all, and a moving query without one is searched again."""
    pb, pts, nor, poses, thresh, ref = _placed_rounds(orc, place)
    nn_method, opts = ROUND_METHODS[method]
    engs = []
    try:
        for cache in (1, 0):
            e = mvicp.Engine(0)
            engs.append(e)
            e.set_option("nn_cache", cache); e.set_option("list_reuse", cache)
            for k, v in opts.items():
                e.set_option(k, v)
            e.set_frames(pts, nor); e.set_graph(pb["src"], pb["dst"])
            e.profile(True); e.set_option("nn_census", 1)
        hit_frac = []
        for r, P in enumerate(poses):
            res = []
            for e in engs:
                e.profile_reset()
                c, w = e.correspond(P, pb["fixed"], thresh, nn_method)
                res.append((c, w, [e.get_correspondences(k) for k in range(e.E)], e.nn_census()))
            (c1, w1, l1, s1), (c0, w0, l0, s0) = res
            assert np.array_equal(c1, c0) and w1.tobytes() == w0.tobytes(), (place, method, r)
            for k, (a, b) in enumerate(zip(l1, l0)):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (place, method, r, k)
            assert s0["hits"] == 0
            hit_frac.append(s1["hits"] / s1["queries"])
            if r in ref:
                for k, (f, sec, dist, wt, _, _) in enumerate(ref[r]):
                    assert c1[k] == len(f), (place, method, r, k)
                    assert np.array_equal(l1[k][0], f) and np.array_equal(l1[k][1], sec) and np.array_equal(l1[k][2], dist), (place, method, r, k)
                    assert w1[k] == (wt if len(f) else 0), (place, method, r, k)
        print("offorigin rounds %-10s %-6s hit fraction per round: %s" % (place, method, " ".join("%.3f" % h for h in hit_frac)))
        if method == "grid" and place != "utm_apart":
            assert hit_frac[len(MAGS)] > 0.5, (place, hit_frac)
    finally:
        for e in engs:
            e.close()


# ---------------------------------------------------------------- d. queries on bisector planes
STEPS = [3e-10, 1e-10, 3e-11]
BISECTOR_CUTOFF = np.float32(0.004)


@pytest.mark.parametrize("T", [0.0, 1e6, 4e6])
def test_bisector_queries_keep_the_right_neighbour_after_a_tiny_step(orc, T):
    """The case built for the cache's rounding allowance: 20 000 queries whose best and second-best target are less than a nanometre
    apart in distance, two poses with a common world translation of size T, one pose step of 3e-10 .. 3e-11 between two searches.  The
    fp64 query map moves the queries by ~2^-53 T on top of the step; an allowance that forgets it keeps the old neighbour where the full
    search finds the other one (the formula this test replaced: up to 374 wrong entries of 20 000).  Searched at P (grid
    kernel, and once more with the bounds-leaving tile kernel), then at P @ T_step on the grid kernel: every list is the oracle's and
    the uncached twin's.

    T_step has exactly the nominal size and is applied twice, along +d and -d with d = (1, 1, 1) / sqrt(3) in the lattice's frame: with
    the second-best distance itself as the bound, a step away from the lattice leaves 0.13 of the queries as hits at 3e-10 and a step
    towards it 0.5, so one random direction says little; the mean over the pair (emulated in numpy: 0.39 / 0.75 / 0.89) is free of that.
    At T = 0 the cache must engage: mean hit fraction > 0.25 at every step after a grid search; the tile kernel's bound is its guard
    band, its fraction is printed.  Far from the origin exactness is all that is asked."""
    pts, P, qd = oo.bisector_problem(T, 40 + int(T / 1e6))
    src = np.array([1], dtype=np.int32); dst = np.array([0], dtype=np.int32); fixed = np.array([1, 0], dtype=np.int32)
    # the data first, with numpy only
    block = oo.query_block(P[1], P[0])
    q64 = oo.xf_point(block, pts[1])
    _, best, second = oo.brute_two_nearest(q64, pts[0])
    gap = np.sqrt(second) - np.sqrt(best)
    assert np.mean(gap < 1e-9) > 0.5, np.median(gap)
    dq = q64.astype(oo.LD) - oo.xf_point(block, pts[1], oo.LD)
    err = np.sqrt((dq * dq).sum(1)).astype(np.float64)
    print("bisector T=%g: median gap %.3g, median |q_fp64 - q_longdouble| %.3g" % (T, np.median(gap), np.median(err)))
    if T >= 1e6:
        assert np.mean(err > 1e-11) > 0.5, np.median(err)
    ref0 = orc.correspond_edge(pts[1], P[1], pts[0], P[0], BISECTOR_CUTOFF)
    assert len(ref0[0]) == len(pts[1])
    rng = np.random.default_rng(5)
    d_src = P[1][:3, :3].T @ P[0][:3, :3] @ (np.ones(3) / np.sqrt(3.0))      # d in the source frame's own coordinates
    for step in STEPS:
        frac = {"grid": [], "tile": []}
        for sign in (1.0, -1.0):
            moved = P.copy()
            moved[1] = moved[1] @ oo.exact_step(rng, step, sign * d_src)
            ref1 = orc.correspond_edge(pts[1], moved[1], pts[0], moved[0], BISECTOR_CUTOFF)
            for first in ("grid", "tile"):
                engs = []
                try:
                    for cache in (1, 0):
                        e = mvicp.Engine(0)
                        engs.append(e)
                        e.set_option("nn_cache", cache); e.set_option("list_reuse", cache); e.set_option("tile_bounds", 2)
                        e.set_frames(pts, None); e.set_graph(src, dst)
                        e.profile(True); e.set_option("nn_census", 1)
                    res = []
                    for e in engs:
                        c, w = e.correspond(P, fixed, BISECTOR_CUTOFF, L.NN_GRID if first == "grid" else L.NN_TILE)
                        l0 = e.get_correspondences(0)
                        e.profile_reset()
                        c2, w2 = e.correspond(moved, fixed, BISECTOR_CUTOFF, L.NN_GRID)
                        res.append((c, w, l0, c2, w2, e.get_correspondences(0), e.nn_census()))
                    for which, ref in ((2, ref0), (5, ref1)):
                        f, sec, dist, wt, _, _ = ref
                        for name, got in zip(("cached", "twin"), res):
                            lst = got[which]
                            wrong = int((lst[1] != sec).sum()) if len(lst[1]) == len(sec) else -1
                            assert np.array_equal(lst[0], f) and wrong == 0 and np.array_equal(lst[2], dist), (T, step, sign, first, name, which, wrong)
                            assert got[which - 1][0] == wt, (T, step, sign, first, name, which)
                    assert res[1][6]["hits"] == 0
                    frac[first].append(res[0][6]["hits"] / res[0][6]["queries"])
                finally:
                    for e in engs:
                        e.close()
        print("bisector T=%g step=%g: hit fraction (+d, -d) after a grid search %.3f %.3f, after a tile search %.3f %.3f" % (T, step, *frac["grid"], *frac["tile"]))
        if T == 0.0:
            assert np.mean(frac["grid"]) > 0.25, (step, frac)
