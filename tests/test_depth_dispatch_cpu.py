"""The depth-selected builds of the two tile NN kernels, without a GPU: tests/depthcases.py against the project's sources.

Every arm of the two dispatch lambdas that needs a 3-level target, and every generic arm (a launch of mixed depths), has a case in
depthcases.VARIANTS; every entry names an arm that exists; the restated `levels(n)` sits on both sides of every boundary; and every
case generator has the properties it states (size, exact ties, duplicates)."""
import numpy as np
import pytest

import depthcases as dc


def test_constants_and_levels_on_both_sides_of_every_boundary():
    k = dc.CONSTANTS
    assert k == {"LEAF": 32, "FAN": 64}, k          # the sizes below are written for these
    assert [dc.levels(n) for n in (1, 32, 33, 2048, 2049, 131072, 131073, 133121, 8388608, 8388609)] == [1, 1, 1, 1, 2, 2, 3, 3, 3, 4]
    assert dc.N3 == 131073 and dc.RAGGED_SIZES == (131073, 131105, 133121)
    assert dc.levels(dc.N3 - 1) == 2 and all(dc.levels(n) == 3 for n in dc.RAGGED_SIZES + dc.SINGLE_SIZES + (dc.ROUNDS_TARGET,))
    assert [dc.levels(n) for n in dc.MIXED_SIZES] == [3, 2, 1]
    # the ragged end: the last tile of every size holds one point; the top node has two children, the second with 1, 1 and 2 boxes
    for n, boxes in zip(dc.RAGGED_SIZES, (1, 1, 2)):
        tiles = -(-n // k["LEAF"])
        assert n - (tiles - 1) * k["LEAF"] == 1
        l1 = -(-tiles // k["FAN"])
        assert -(-l1 // k["FAN"]) == 2 and l1 - k["FAN"] == boxes, (n, tiles, l1)


def test_every_depth_3_and_generic_arm_has_a_case_and_every_case_an_arm():
    need = dc.required_arms(dc.ARMS)
    assert len(need) >= 25, need
    missing = [a for a in need if a not in dc.VARIANTS]
    assert not missing, "arms of the dispatch without a case in depthcases.VARIANTS: %r" % missing
    unknown = [a for a in dc.VARIANTS if a not in dc.ARMS]
    assert not unknown, "cases in depthcases.VARIANTS that name no arm of the dispatch: %r" % unknown
    for name, v in dc.VARIANTS.items():
        p = dc.parse_launch(name)
        assert p["TOP"] == {3: 2, "mixed": -1, 2: 1}[v["depth"]], name
        assert set(v["opts"]) <= set(dc.OPTION_DEFAULTS), name
        assert v["opts"]["tile_mfma"] == (0 if p["kernel"] == "tile" else 2), name
        if p["kernel"] == "mfma":
            assert p["CEN"] == v["census"], name
        assert p["BND"] == (1 if v["opts"].get("tile_bounds") == 2 else 0), name
    # what the GPU test can run through the one-edge route, and what only a moving round reaches
    assert [k for k, v in dc.VARIANTS.items() if v["round"] == "cached"] == ["mfma<5,2,1,0,1,0>"]


def test_the_check_fails_on_a_removed_case_and_on_an_added_arm():
    """Both directions once, on edited copies: the table without one entry, and the sources with one more arm."""
    need = dc.required_arms(dc.ARMS)
    table = dict(dc.VARIANTS)
    del table["mfma<5,2,1,0,0,1>"]
    assert [a for a in need if a not in table] == ["mfma<5,2,1,0,0,1>"]
    tile = dc.read_source("nn_tile.hip")
    more = tile.replace("    else if (top == 2 && waves == 8) MVICP_TILE_K(8, 2, false);", "    else if (top == 2 && waves == 8) MVICP_TILE_K(8, 2, false);\n    else if (top == 2 && waves == 5) MVICP_TILE_K(5, 2, false);")
    assert more != tile
    assert [a for a in dc.required_arms(dc.tile_arms(more)) if a not in dc.VARIANTS] == ["tile<5,2,0>"]
    mfma = dc.read_source("nn_mfma.hip")
    more = mfma.replace("    else if (top == 2 && waves == 4) MVICP_MFMA_K(4, 2, false);", "    else if (top == 2 && waves == 4) MVICP_MFMA_K(4, 2, false);\n    else if (top == 2 && waves == 3) MVICP_MFMA_L(3, 2, false, false, true);")
    assert more != mfma
    assert [a for a in dc.required_arms(dc.mfma_arms(more)) if a not in dc.VARIANTS] == ["mfma<3,2,0,0,1,0>"]
    # an arm that launches without naming itself, a renamed dispatch, a constant that is gone: a LookupError, not a shorter list
    raw = tile.replace("    else MVICP_TILE_K(6, -1, false);", "    else hipLaunchKernelGGL((nn_tile_kernel<6, -1, false>), grid, dim3(TT), 0, c->stream, d_jobs, d2_bound, search_bound(c, d2_bound), d_stats);")
    assert raw != tile
    for bad, fn in ((raw, dc.tile_arms), (tile.replace("int launch_nn_tile_edges(", "int launch_tiles("), dc.tile_arms),
                    (mfma.replace("MVICP_MFMA_E(5, 2, true, false);", "MVICP_MFMA_E(5, top, true, false);"), dc.mfma_arms),
                    (dc.read_source("nn_tile_common.h").replace("constexpr int FAN = 64;", "constexpr int FANOUT = 64;"), dc.tile_constants)):
        with pytest.raises(LookupError):
            fn(bad)
    with pytest.raises(ValueError):
        dc.parse_launch("tile<7,2>")
    assert dc.parse_launch("mfma<5,-1,1,0,0,1>") == {"kernel": "mfma", "WPE": 5, "TOP": -1, "BND": 1, "CEN": 0, "LBT": 0, "ENTRY": 1}
    assert dc.parse_launch("grid") == {"kernel": "grid"}


def _brute(q, dst):
    """(lowest index at the best distance, best d2, how many targets are at exactly that distance), in the reference's operation order"""
    d2 = dc.dist2(q[:, None, :], dst[None])
    best = d2.min(axis=1)
    return np.argmax(d2 == best[:, None], axis=1), best, (d2 == best[:, None]).sum(axis=1)


def test_single_query_cases_have_the_stated_sizes_and_query_mix():
    for kind, places in dc.SINGLE_PLACES.items():
        assert set(places) >= {"local", "mm_local"}
    assert {k for k, p in dc.SINGLE_PLACES.items() if "utm" in p and "local1e6" in p} == {"blob", "lattice"}
    nq = dc.N_OTHER + dc.N_NEAR + dc.N_BLOB + 2
    assert 1500 <= nq <= 1700 and nq % 64 != 0, nq          # about 1600 queries, a ragged last wave
    for place, kind, n in (("mm_local", "lattice", dc.SINGLE_SIZES[0]), ("utm", "blob", dc.SINGLE_SIZES[1])):
        dst, q = dc.single_query_case(place, kind, n)
        assert dst.shape == (n, 3) and q.shape == (nq, 3) and dc.levels(len(dst)) == 3
        s = dc.oo.place_scale(place)
        near = q[dc.N_OTHER:dc.N_OTHER + dc.N_NEAR]
        _, best, _ = _brute(near[:16], dst)
        assert np.all(best <= 3.1 * (1e-9 * s) ** 2 * 1.0001 + (np.abs(dst).max() * 2.0 ** -52) ** 2 * 12), best.max()   # beside a target point: 1e-9 s per axis + rounding
        far = q[-2:]
        assert np.all(np.sqrt(_brute(far, dst)[1]) > 100 * s)
        dst2, q2 = dc.single_query_case(place, kind, n)
        assert np.array_equal(dst, dst2) and np.array_equal(q, q2)          # seeded


def test_lattice_case_has_exact_ties_and_near_ties():
    dst, q, ties = dc.lattice_tie_case()
    assert dst.shape == (363 * 362, 3) and len(dst) == 131406 and dc.levels(len(dst)) == 3 and len(q) == len(ties) == 1200
    counts = [len(t) for t in ties]
    assert counts.count(1) == 300 and counts.count(2) == 300 and counts.count(4) == 300 and counts.count(0) == 300
    for j, t in enumerate(ties):
        if len(t) > 1:
            d = dc.dist2(q[j], dst[list(t)])
            assert np.all(d == d[0]) and d[0] > 0, (j, d)          # exactly equal distances, in the kernels' operation order
        elif len(t) == 1:
            assert dc.dist2(q[j], dst[t[0]]) == 0.0
    # against the whole lattice, on a sample of every kind: the stated targets are THE nearest ones, and no others tie
    for k in range(4):
        sl = slice(300 * k, 300 * k + 24)
        low, best, nbest = _brute(q[sl], dst)
        for j, t in enumerate(ties[sl]):
            if t:
                assert nbest[j] == len(t) and low[j] == min(t) and best[j] == dc.dist2(q[sl][j], dst[t[0]]), (k, j)
            else:
                assert nbest[j] == 1
                d2 = np.sort(dc.dist2(q[sl][j], dst))[:2]
                assert np.sqrt(d2[1]) - np.sqrt(d2[0]) < 1e-9          # bisector queries: best and second best less than a nanometre apart


def test_duplicate_case_stores_every_point_twice():
    dst, q = dc.duplicate_case()
    assert len(dst) == 2 * dc.N_UNIQUE == 131074 and dc.levels(len(dst)) == 3 and len(q) == 1200
    u, inverse, counts = np.unique(dst, axis=0, return_inverse=True, return_counts=True)
    assert len(u) == dc.N_UNIQUE and np.all(counts == 2)
    first = np.full(len(u), -1); second = np.full(len(u), -1)
    for i, g in enumerate(np.ravel(inverse)):
        if first[g] < 0:
            first[g] = i
        else:
            second[g] = i
    assert np.mean(second - first == dc.N_UNIQUE) < 0.01          # unrelated indices, not i and i + n
    low, best, nbest = _brute(q[:16], dst)
    assert np.all(best == 0.0) and np.all(nbest == 2)
    low, best, nbest = _brute(q[400:416], dst)
    assert np.all(best > 0.0) and np.all(nbest == 2)


def test_ragged_mixed_and_rounds_cases_have_the_stated_sizes():
    dst = dc.ragged_target(dc.RAGGED_SIZES[0])
    assert dst.shape == (dc.N3, 3)
    q, mine = dc.ragged_queries(dst, [17], 1200)
    assert mine == 10 and len(q) == 10 + 1200 + 3 and len(q) % 64 != 0
    assert np.array_equal(q[0], dst[17]) and np.all(np.abs(q[1:10] - dst[17]).max(axis=1) <= 1.0000001e-9 + 1e-12)
    targets, qm = dc.mixed_case()
    assert [len(t) for t in targets] == list(dc.MIXED_SIZES) and len(qm) == 1602 and len(qm) % 64 != 0
    pb = dc.rounds_problem()
    assert [len(p) for p in pb["pts"]] == [140000, 4000, 4000] and [n.shape for n in pb["nor"]] == [p.shape for p in pb["pts"]]
    assert list(pb["src"]) == [1, 2] and list(pb["dst"]) == [0, 0] and list(pb["fixed"]) == [1, 0, 0]
    assert len(dc.ROUNDS_MAGS) + 2 == 8 and len(dc.ROUNDS_MAGS_SETTLED) + 2 == 8
