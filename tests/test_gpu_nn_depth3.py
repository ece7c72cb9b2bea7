"""The builds of nn_tile_kernel and nn_mfma_kernel that exist for 3-level targets only (more than 131 072 points: what bench.py measures
at cfg4 and cfg5), on adversarial inputs: every case asserts that the target has 3 box levels, that the intended instantiation was
launched (Engine.last_nn_launch) and the oracle's bytes — the real nanoflann (oracle/_ref) for the indices, the oracle's brute force for
the distances.  tests/depthcases.py holds the table launch string -> (options, method, kind of round) and the case generators;
tests/test_depth_dispatch_cpu.py holds that table against the dispatch source.

An arbitrary query set reaches a tile kernel as the source cloud of one edge (mvicp_nn_query maps the tile methods to the grid kernel):
target = frame 0, queries = frame 1, identity poses (the query map is exact), a cutoff above every distance.

Left out: targets of 4 and 5 levels (more than 8 388 608 points), and the geometric-progression clouds of test_gpu_deep_tie.py."""
import numpy as np
import pytest

import depthcases as dc
import mvicp
import offorigin as oo
from mvicp import lib as L

pytestmark = pytest.mark.gpu


def _levels(e, frame):
    return int(e.get_structure(frame, "scalars")[13])          # wide_levels


def _check_lists(e, counts, weights, expected, tag):
    """every edge's list, count and weight against (first, second, dist, weight)"""
    for k, (f, s, d, w) in enumerate(expected):
        gf, gs, gd = e.get_correspondences(k)
        assert counts[k] == len(f) and len(gf) == len(f), (tag, k, int(counts[k]), len(f))
        bad = np.nonzero((gs != s) | (gd != d) | (gf != f))[0]
        assert len(bad) == 0, (tag, k, len(bad), bad[:5].tolist(), gs[bad[:5]].tolist(), s[bad[:5]].tolist(), gd[bad[:5]].tolist(), d[bad[:5]].tolist())
        assert weights[k] == w, (tag, k)


def _oracle(orc, refnn, dst, q, lowest=False):
    """(idx, d2): the oracle's distances, the real nanoflann's indices (lowest = True: the oracle's lowest index)"""
    assert refnn is not None, "oracle/_ref (real nanoflann) was not built"
    oi, od = orc.nn_brute(dst, q)
    ri, rd = refnn.query(dst, q)
    assert np.array_equal(rd, od)
    return (oi if lowest else ri), od, int((ri != oi).sum())


def _engine(frames, src, dst, nor=None, opts=None):
    e = mvicp.Engine(0)
    for k, v in (opts or {}).items():
        e.set_option(k, v)
    e.set_frames(frames, nor); e.set_graph(src, dst)
    return e


def _run_variants(e, names, poses, fixed, thresh, expected, tag, depth=3):
    """every named variant of the table on one engine: each search equals the oracle, the variant's last search is the named build"""
    seen = set()
    for name in names:
        v = dc.VARIANTS[name]
        assert v["depth"] == depth, name
        launch = None
        for r, c, w, launch in dc.search_variant(e, v, poses, fixed, thresh):
            assert dc.parse_launch(launch)["TOP"] == dc.parse_launch(name)["TOP"], (tag, name, r, launch)
            _check_lists(e, c, w, expected, (tag, name, r, launch))
            seen.add(launch)
        assert launch == name, (tag, name, launch)
    return seen


# ---------------------------------------------------------------- a. single queries through every depth-3 build
SINGLE_CASES = [(place, kind, n) for kind in dc.KINDS for place in dc.SINGLE_PLACES[kind] for n in dc.SINGLE_SIZES]
SINGLE_VARIANTS = [k for k, _ in dc.variants(3)]


_SINGLE = {}


def _single_case(orc, refnn, key):
    """the case and its oracle, shared by the two halves of the variant list (the last case only: a target is 3.6 MB)"""
    if _SINGLE.get("key") != key:
        dst, q = dc.single_query_case(*key)
        idx, d2, _ = _oracle(orc, refnn, dst, q)
        _SINGLE.update(key=key, value=(dst, q, idx, d2))
    return _SINGLE["value"]


@pytest.mark.parametrize("place,kind,n", SINGLE_CASES)
@pytest.mark.parametrize("half", [0, 1])
def test_single_queries_through_every_depth_3_build(orc, refnn, half, place, kind, n):
    """Targets of 131 073 and 150 000 points (blob, plane, lattice, clusters; local and millimetre site frames, blob and lattice also at
    1e6 m and at UTM coordinates), 1602 queries — another cloud, target points +- 1e-9 of the data scale, a blob, two far ones — through
    every build of the table that a first or a repeated search reaches: unseeded and seeded, tile_waves 6 / 8 and 4 / 6, mfma_lbt 0,
    mfma_entry with and without bounds, the census builds, the bounds-leaving builds.  In two halves (every other entry of the table):
    the query 1e6 m above a millimetre plane ties with all 131 073 targets, and the fix-up that walks the reference's tree for it takes
    0.2 s per search."""
    dst, q, idx, d2 = _single_case(orc, refnn, (place, kind, n))
    names = SINGLE_VARIANTS[half::2]
    thresh = dc.cutoff_above(d2)
    frames, src, dsts, poses, fixed = dc.edge_frames([dst], q)
    e = _engine(frames, src, dsts)
    try:
        assert _levels(e, 0) == 3
        seen = _run_variants(e, names, poses, fixed, thresh, [dc.expected_list(orc, idx, d2, thresh)], (place, kind, n))
        assert seen >= set(names)
    finally:
        e.close()


def test_the_cases_of_this_file_reach_every_build_of_the_table():
    """(no launch) every entry for 3-level targets is run by (a), except the one a moving round reaches, which (d) and (e) assert"""
    assert set(SINGLE_VARIANTS) | set(CACHED_ARMS) == {k for k, v in dc.VARIANTS.items() if v["depth"] == 3}
    assert set(MIXED_VARIANTS) == {k for k, v in dc.VARIANTS.items() if v["depth"] == "mixed"}


# ---------------------------------------------------------------- b. the ragged end of the tree
RAGGED_VARIANTS = ["tile<7,2,0>", "tile<6,2,0>", "tile<6,2,1>", "mfma<5,2,0,0,1,0>", "mfma<5,2,0,0,0,0>", "mfma<5,2,0,1,0,0>", "mfma<5,2,1,0,0,0>", "mfma<5,2,1,1,0,0>",
                   "mfma<5,2,0,0,0,1>", "mfma<5,2,1,0,0,1>"]


@pytest.mark.parametrize("n", dc.RAGGED_SIZES)
def test_ragged_last_node_last_tile_last_point(orc, refnn, n):
    """131 073, 131 105 and 133 121 points: the top node has two children, the second one 1, 1 and 2 boxes, and the last tile one point.
    Queries on and +- 1e-9 beside the points of the last two tiles (found through the structure's own `sidx`), next to queries across the
    rest of the cloud; both kernels, unseeded and seeded, plain and bounds-leaving."""
    dst = dc.ragged_target(n)
    leaf = dc.CONSTANTS["LEAF"]
    e = mvicp.Engine(0)
    try:
        e.set_frames([dst], None)
        sidx = e.get_structure(0, "sidx").view(np.int32)
        assert len(sidx) == n and _levels(e, 0) == 3
        tiles = -(-n // leaf)
        last = sidx[(tiles - 2) * leaf:]
        assert len(last) == leaf + 1
        q, mine = dc.ragged_queries(dst, last)
        assert mine == 10 * (leaf + 1) and len(q) % 64 != 0
        idx, d2, _ = _oracle(orc, refnn, dst, q)
        assert np.array_equal(idx[:mine:10], last)          # the queries ON the last tiles' points find exactly them
        thresh = dc.cutoff_above(d2)
        frames, src, dsts, poses, fixed = dc.edge_frames([dst], q)
        e.set_frames(frames, None); e.set_graph(src, dsts)
        assert _levels(e, 0) == 3 and np.array_equal(e.get_structure(0, "sidx").view(np.int32), sidx)
        _run_variants(e, RAGGED_VARIANTS, poses, fixed, thresh, [dc.expected_list(orc, idx, d2, thresh)], ("ragged", n))
    finally:
        e.close()


# ---------------------------------------------------------------- c. ties and duplicates
TIE_VARIANTS = ["tile<7,2,0>", "tile<6,2,0>", "tile<6,2,1>", "mfma<5,2,0,0,1,0>", "mfma<5,2,0,0,0,0>", "mfma<5,2,0,1,0,0>", "mfma<5,2,1,0,0,0>", "mfma<5,2,0,0,0,1>"]


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("case", ["lattice", "duplicates"])
def test_ties_and_duplicates_under_a_3_level_tree(orc, refnn, case, lazy):
    """A 363 x 362 lattice with queries on its points, exactly between two and four of them and within 3e-10 of a bisector plane, and a
    cloud of 65 537 points each stored twice: with "tie_rule" 1 every answer is the real nanoflann's, with "tie_rule" 0 the lowest index;
    with the reference-equivalent trees built lazily (the default) and at mvicp_set_graph."""
    if case == "lattice":
        dst, q, _ = dc.lattice_tie_case()
    else:
        dst, q = dc.duplicate_case()
    ref_idx, d2, differ = _oracle(orc, refnn, dst, q)
    low_idx, _, _ = _oracle(orc, refnn, dst, q, lowest=True)
    assert differ > 0, "the data must make the two tie rules disagree"
    thresh = dc.cutoff_above(d2)
    frames, src, dsts, poses, fixed = dc.edge_frames([dst], q)
    e = _engine(frames, src, dsts, opts={"tie_lazy": lazy})
    try:
        assert _levels(e, 0) == 3
        for rule, idx in ((1, ref_idx), (0, low_idx), (1, ref_idx)):
            e.set_option("tie_rule", rule)
            _run_variants(e, TIE_VARIANTS, poses, fixed, thresh, [dc.expected_list(orc, idx, d2, thresh)], (case, lazy, rule))
    finally:
        e.close()


# ---------------------------------------------------------------- d. cached rounds
BASE_T0 = {"tile_mfma": 0, "tile_bounds": 2, "tile_cache": 2}
BASE_T2 = {"tile_mfma": 2, "tile_bounds": 2, "tile_cache": 2}
# name -> (method, options, census on, the builds that must have been launched, where the script starts: depthcases.placed_rounds)
ROUND_CONFIGS = {
    "tile0_miss0": (L.NN_TILE, dict(BASE_T0, tile_miss=0), 1, {"tile<6,2,1>"}, "init"),
    "tile0_miss64": (L.NN_TILE, dict(BASE_T0, tile_miss=64), 1, {"tile<6,2,1>"}, "init"),
    "tile0_noreject": (L.NN_TILE, dict(BASE_T0, reject_cache=0), 1, {"tile<6,2,1>"}, "init"),
    "tile2": (L.NN_TILE, dict(BASE_T2), 1, {"mfma<5,2,1,1,0,0>"}, "init"),
    "tile2_noreject": (L.NN_TILE, dict(BASE_T2, reject_cache=0), 1, {"mfma<5,2,1,1,0,0>"}, "init"),
    "tile2_lbt2": (L.NN_TILE, dict(BASE_T2, mfma_lbt=2), 0, {"mfma<5,2,1,0,0,0>", "mfma<5,2,1,0,1,0>"}, "init"),
    "tile2_lbt2_miss64": (L.NN_TILE, dict(BASE_T2, mfma_lbt=2, tile_miss=64, reject_cache=0), 0, {"mfma<5,2,1,0,0,0>", "mfma<5,2,1,0,1,0>"}, "init"),
    # AUTO picks the kernel of a cache-aware round from the queries' displacement bound in guard bands ("cache_mfma_ratio"; millimetre data at
    # UTM coordinates stays on the matrix pipe throughout): the second row pins those rounds to nn_tile_kernel, every wave through miss_block
    "auto": (L.NN_AUTO, {}, 1, {"mfma<5,2,0,1,1,0>", "mfma<5,2,1,1,0,0>", "grid"}, "gt"),
    "auto_tile_miss64": (L.NN_AUTO, {"tile_miss": 64, "cache_mfma_ratio": 0}, 1, {"mfma<5,2,1,1,0,0>", "tile<6,2,1>", "grid"}, "gt"),
}
CACHED_ARMS = ["mfma<5,2,1,0,1,0>"]
ORACLE_ROUNDS = (0, 3, 7)
_PLACED = {}


def _placed(orc, refnn, place, start):
    """the placed problem and the oracle's lists of rounds 0, 3 and 7: once per placement.  The queries are the restated query map's
    (offorigin.xf_point), so that the real nanoflann answers them; round 0 is held against the oracle's brute force over the whole edge, bit
    for bit (4000 x 140 000 distances per edge cost a second and a half: once per edge, not once per round)."""
    if (place, start) not in _PLACED:
        assert refnn is not None, "oracle/_ref (real nanoflann) was not built"
        pb, pts, nor, poses, thresh = dc.placed_rounds(place, start)
        ref = {}
        for r in ORACLE_ROUNDS:
            ref[r] = []
            for s, d in zip(pb["src"], pb["dst"]):
                qx = np.ascontiguousarray(oo.xf_point(oo.query_block(poses[r][s], poses[r][d]), pts[s]))
                ri, rd = refnn.query(pts[d], qx)
                lst = orc.filter_median(ri, rd, thresh)
                if r == 0:          # the restated map and nanoflann's distances are the oracle's own, bit for bit: the whole-edge brute force agrees
                    f, sec, dist, wt, _, od = orc.correspond_edge(pts[s], poses[r][s], pts[d], poses[r][d], thresh)
                    assert np.array_equal(rd, od) and np.array_equal(f, lst[0]) and np.array_equal(dist, lst[2]) and wt == lst[3]
                ref[r].append(lst)
        _PLACED[(place, start)] = (pb, pts, nor, poses, thresh, ref)
    return _PLACED[(place, start)]


@pytest.mark.parametrize("config", list(ROUND_CONFIGS))
@pytest.mark.parametrize("place", dc.ROUNDS_PLACES)
def test_cached_rounds_under_a_3_level_tree_equal_the_uncached_twin(orc, refnn, place, config):
    """One target of 140 000 points, two sources of 4000 (bumpy-sphere views, at unit scale and in millimetres at UTM coordinates), the
    eight scripted rounds of offorigin.scripted_poses (3e-3 .. 1e-7 and the last poses once more, from the noisy initial poses, for the
    TILE method; 1e-3 .. 1e-6 from the ground truth for AUTO, which runs cache-aware rounds only while the queries lie within 1.5 hash
    cells of the target: depthcases.ROUNDS_MAGS_SETTLED) beside a twin without temporal cache and
    list reuse: counts, weights and lists are the twin's after every round and the real nanoflann's after rounds 0, 3 and 7.  Every tile
    launch is a 3-level build, the config's builds were launched, and where the census counts at least two rounds have a hit fraction
    strictly between 0.02 and 0.98 (the bar of test_cfg4_moving_rounds_cache_and_list_reuse_are_bit_identical): the cache prologue and
    the search of the missed lanes both ran."""
    method, opts, census, want, start = ROUND_CONFIGS[config]
    pb, pts, nor, poses, thresh, ref = _placed(orc, refnn, place, start)
    engs = []
    try:
        for cache in (1, 0):
            e = _engine(pts, pb["src"], pb["dst"], nor, dict(opts, nn_cache=cache, list_reuse=cache))
            engs.append(e)
            e.profile(bool(census)); e.set_option("nn_census", census)
        assert _levels(engs[0], 0) == 3 and _levels(engs[1], 0) == 3
        hit_frac, launches = [], []
        for r, P in enumerate(poses):
            res = []
            for e in engs:
                e.profile_reset()
                c, w = e.correspond(P, pb["fixed"], thresh, method)
                res.append((c, w, [e.get_correspondences(k) for k in range(e.E)], e.nn_census(), e.last_nn_launch()))
            (c1, w1, l1, s1, n1), (c0, w0, l0, s0, n0) = res
            launches.append(n1)
            for n in (n1, n0):
                assert dc.parse_launch(n).get("TOP", 2) == 2, (place, config, r, n)
            assert np.array_equal(c1, c0) and w1.tobytes() == w0.tobytes(), (place, config, r)
            for k, (a, b) in enumerate(zip(l1, l0)):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (place, config, r, k)
            if census:
                assert s0["hits"] == 0
                hit_frac.append(s1["hits"] / s1["queries"])
            if r in ref:
                _check_lists(engs[0], c1, w1, ref[r], (place, config, r))
        print("depth3 rounds %-7s %-18s launches: %s" % (place, config, " ".join(launches)))
        print("depth3 rounds %-7s %-18s hit fraction per round: %s" % (place, config, " ".join("%.3f" % h for h in hit_frac)))
        assert want <= set(launches), (place, config, launches)
        if census:
            assert sum(0.02 < h < 0.98 for h in hit_frac) >= 2, (place, config, hit_frac)
    finally:
        for e in engs:
            e.close()


# ---------------------------------------------------------------- e. the option rows that a 2-level target cannot tell apart
# (options, the build the row is for).  The rows of test_gpu_parity.py:test_tuning_options_never_change_results whose arm needs a 3-level
# target, and "mfma_lbt" 2.  Under AUTO with the default "tile_mfma" 1 nn_tile_kernel runs only in cache-aware rounds (always its
# bounds-leaving 6-wave build), so "tile_waves" 8 selects nothing there at any depth: its arm needs "tile_mfma" 0 beside it.
OPTION_ROWS = [
    ({"tile_waves": 4}, "mfma<4,2,0,0,0,0>"),
    ({"tile_mfma": 2, "tile_waves": 4}, "mfma<4,2,0,0,0,0>"),
    ({"tile_mfma": 2, "tile_waves": 6}, "mfma<6,2,0,0,0,0>"),
    ({"tile_waves": 8}, None),
    ({"tile_mfma": 0, "tile_waves": 8}, "tile<8,2,0>"),
    ({"tile_mfma": 0, "tile_waves": 6}, "tile<6,2,0>"),
    ({"tile_mfma": 0}, "tile<7,2,0>"),
    ({"mfma_lbt": 0}, "mfma<5,2,0,0,0,0>"),
    ({"mfma_entry": 1}, "mfma<5,2,0,0,0,1>"),
    ({"mfma_entry": 1, "tile_bounds": 2}, "mfma<5,2,1,0,0,1>"),
    ({"mfma_entry": 1, "tile_seed": 0}, "mfma<5,2,0,0,1,0>"),
    ({"tile_mfma": 2, "tile_bounds": 2, "tile_cache": 2, "mfma_lbt": 2}, "mfma<5,2,1,0,1,0>"),
    ({"tile_mfma": 2, "mfma_lbt": 2}, "mfma<5,2,1,0,1,0>"),
]
_TRAJECTORY = {}


def _trajectory(options):
    """7 AUTO rounds with solves on the problem of (d) at unit scale -> (per round: counts, weights, lists; final poses; launches)"""
    pb, pts, nor, poses, thresh = _TRAJECTORY.setdefault("problem", dc.placed_rounds("unit"))
    e = _engine(pts, pb["src"], pb["dst"], nor, options)
    try:
        assert _levels(e, 0) == 3
        P = poses[0].copy()
        trace, launches = [], []
        for r in range(7):
            c, w = e.correspond(P, pb["fixed"], thresh, L.NN_AUTO)
            launches.append(e.last_nn_launch())
            trace.append((c.copy(), w.copy(), [e.get_correspondences(k) for k in range(e.E)]))
            P, sm = e.optimize(P, pb["fixed"], L.PARAM_SOPHUS_SE3, 1, True, 50)
        return trace, P, launches
    finally:
        e.close()


@pytest.mark.parametrize("opts,arm", OPTION_ROWS, ids=lambda x: "-".join("%s%g" % kv for kv in x.items()) if isinstance(x, dict) else str(x))
def test_tuning_options_never_change_results_on_a_3_level_target(opts, arm):
    """The whole trajectory (counts, weights, every list of every round, the final poses) is bit-identical to the default's, and the
    build the row is for was launched in one of the rounds."""
    if "base" not in _TRAJECTORY:
        _TRAJECTORY["base"] = _trajectory({})
    base_trace, base_poses, base_launches = _TRAJECTORY["base"]
    trace, P, launches = _trajectory(opts)
    print("depth3 options %s: %s (default: %s)" % (opts, " ".join(launches), " ".join(base_launches)))
    for r, ((c0, w0, l0), (c1, w1, l1)) in enumerate(zip(base_trace, trace)):
        assert np.array_equal(c0, c1) and w0.tobytes() == w1.tobytes(), (opts, r)
        for a, b in zip(l0, l1):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (opts, r)
    assert np.array_equal(base_poses, P), opts
    if arm is not None:
        assert arm in launches, (opts, arm, launches)
    for n in launches:
        assert dc.parse_launch(n).get("TOP", 2) == 2, (opts, n)


# ---------------------------------------------------------------- f. mixed depths in one launch
MIXED_VARIANTS = [k for k, _ in dc.variants("mixed")]


def test_mixed_depths_in_one_launch_run_the_generic_builds(orc, refnn):
    """Targets of 131 073, 3000 and 500 points (3, 2 and 1 levels) in one graph: the generic builds walk each from its own top level
    (case 2, case 1, case 0).  Both kernels, plain, bounds-leaving and counting, against the real nanoflann."""
    targets, q = dc.mixed_case()
    answers = [_oracle(orc, refnn, t, q)[:2] for t in targets]
    thresh = dc.cutoff_above(np.concatenate([d2 for _, d2 in answers]))
    expected = [dc.expected_list(orc, idx, d2, thresh) for idx, d2 in answers]
    frames, src, dsts, poses, fixed = dc.edge_frames(targets, q)
    e = _engine(frames, src, dsts)
    try:
        assert [_levels(e, k) for k in range(3)] == [3, 2, 1]
        seen = _run_variants(e, MIXED_VARIANTS, poses, fixed, thresh, expected, "mixed", depth="mixed")
        assert seen >= set(MIXED_VARIANTS)
    finally:
        e.close()
