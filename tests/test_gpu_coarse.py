"""mvicp_coarse_pairs / mvicp_coarse_pairs_fetch (and mvicp.init_from_clouds on top of them) on the MI355X: every field of every edge's
record and every fetched pair and flag equals BOTH the loop of today's single-pair calls (Engine.feature_match -> match_pairs -> the
gather -> Engine.consensus) and the numpy statement of that chain (tests/matchref.py through tests/initref.py), byte for byte; no
tolerance anywhere.  What the cases must contain (pair counts of 0, 2, 3 and 257, ties, a reversed and a repeated edge, rejected edges) is
asserted on the reference alone, so no case can pass trivially."""
import ctypes as C
import functools

import numpy as np
import pytest

import initref as ir
import matchref as mr
import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
SET_ROWS = (0, 1, 2, 63, 64, 65, 257, 300, 3)
# (i, j), (j, i) and a repeated edge; every set size on either side; empty sets on either side
EDGES = ((6, 7), (7, 6), (6, 7), (3, 4), (4, 5), (5, 3), (0, 7), (7, 0), (1, 7), (2, 7), (8, 7), (7, 8), (2, 1), (5, 6), (3, 7), (1, 2))
SEEDS = tuple([11, 12, 2 ** 64 - 1, 14, 15, 16, 17, 18, 19, 20, 2 ** 63, 22, 23, 24, 25, 26])
TAU, EDGE_SIM = 0.05, 0.8


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    e.set_option("match_chunk", 64)   # (chunks end inside tiles at these sizes: 257 = 4 x 64 + 1, 300 = 4 x 64 + 44, 65 = 64 + 1)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def sets(dim):
    """-> (desc (total, dim), xyz (total, 3), offsets).  One base table of integer-valued descriptors (exact ties, first and second place
    alike) and one base cloud; set s holds the first rows of both, the cloud moved by a pose of its own, a sixth of its rows with another
    row's descriptor and a little noise on its points: matches are mostly i <-> i, so hypotheses are accepted and the counts differ."""
    rng = np.random.Generator(np.random.PCG64(1000 + dim))
    base_d = rng.integers(0, 3, size=(300, dim)).astype(np.float64)
    base_x = rng.uniform(0.0, 1.0, size=(300, 3))
    desc, xyz = [], []
    for n in SET_ROWS:
        d, x = base_d[:n].copy(), base_x[:n].copy()
        swap = rng.random(n) < 1.0 / 6.0
        d[swap] = base_d[rng.integers(0, 300, size=int(swap.sum()))]
        R, t = synth.so3_exp(rng.uniform(-1.0, 1.0, size=3)), rng.uniform(-0.5, 0.5, size=3)
        desc.append(d); xyz.append(x @ R.T + t + rng.normal(0.0, 0.01, size=(n, 3)))
    offsets = np.concatenate([[0], np.cumsum(SET_ROWS)]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(desc)), np.ascontiguousarray(np.concatenate(xyz)), offsets


def rows(arr, offsets, s):
    return np.ascontiguousarray(arr[offsets[s]:offsets[s + 1]])


@functools.lru_cache(maxsize=None)
def reference(dim, mutual, ratio, H):
    """the numpy chain per edge of EDGES"""
    desc, xyz, off = sets(dim)
    return [ir.coarse_edge(rows(desc, off, a), rows(xyz, off, a), rows(desc, off, b), rows(xyz, off, b), mutual, ratio, H, seed, TAU, EDGE_SIM)
            for (a, b), seed in zip(EDGES, SEEDS)]


def single_calls(eng, desc, xyz, off, edges, seeds, mutual, ratio, H, tau, edge_sim):
    """the loop of today's calls per edge -> the same dicts as ir.coarse_edge"""
    out = []
    for (a, b), seed in zip(edges, seeds):
        mt = eng.feature_match(rows(desc, off, a), rows(desc, off, b))
        pairs = mvicp.match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, ratio)
        c = len(pairs)
        rec = {"pairs_n": c, "best": -1, "count": 0, "accepted": 0, "pose": np.eye(4), "pairs": pairs, "flags": np.zeros(c, dtype=np.uint8)}
        if c >= 3:
            P, Q = np.ascontiguousarray(rows(xyz, off, a)[pairs[:, 0]]), np.ascontiguousarray(rows(xyz, off, b)[pairs[:, 1]])
            cons = eng.consensus(P, Q, H, seed, tau, edge_sim)
            rec.update(best=cons["best"], count=cons["count"], accepted=cons["accepted"], pose=cons["pose"], flags=cons["flags"])
        out.append(rec)
    return out


def assert_edges(res, fetch, want, what):
    """res: Engine.coarse_pairs' dict; fetch(e) -> (pairs, flags); want: a list of ir.coarse_edge dicts"""
    assert len(res["pairs"]) == len(want)
    for e, w in enumerate(want):
        for key, ref_key in (("pairs", "pairs_n"), ("best", "best"), ("count", "count"), ("accepted", "accepted")):
            assert res[key].dtype == np.int32 and int(res[key][e]) == int(w[ref_key]), (what, e, key, int(res[key][e]), w[ref_key])
        assert res["pose"][e].tobytes() == np.ascontiguousarray(w["pose"]).tobytes(), (what, e, "pose", res["pose"][e], w["pose"])
        pairs, flags = fetch(e)
        if isinstance(pairs, torch.Tensor):
            pairs, flags = pairs.cpu().numpy(), flags.cpu().numpy()
        assert pairs.dtype == np.int32 and pairs.shape == w["pairs"].shape and pairs.tobytes() == w["pairs"].tobytes(), (what, e, "pairs")
        assert flags.dtype == np.uint8 and flags.shape == w["flags"].shape and flags.tobytes() == w["flags"].tobytes(), (what, e, "flags")


def test_the_cases_contain_what_they_are_for():
    for dim in (33, 7):
        desc, _, off = sets(dim)
        mt = mr.feature_match(rows(desc, off, 6), rows(desc, off, 7))
        assert (mt["fwd_d2"][:, 0] == mt["fwd_d2"][:, 1]).any() and (mt["fwd_d2"][:, 0] < mt["fwd_d2"][:, 1]).any()   # ties and none
    seen = set()
    for mutual in (False, True):
        for ratio in (0.8, 1.0):
            ref = reference(33, mutual, ratio, 255)
            seen |= {r["pairs_n"] for r in ref}
            assert any(r["best"] >= 0 and 0 < r["count"] < r["pairs_n"] for r in ref)   # a winner that is neither empty nor everything
            assert any(r["accepted"] == 0 and r["pairs_n"] >= 3 for r in ref)           # enough pairs and still nothing accepted
            assert any(r["accepted"] > 256 for r in reference(33, mutual, ratio, 2000))  # more than one block of accepted hypotheses
    assert {0, 2, 3, 257} <= seen, sorted(seen)
    ref = reference(33, True, 1.0, 2000)
    assert ref[0]["pairs"].tobytes() != ref[1]["pairs"].tobytes()                     # (i, j) and (j, i) differ
    assert ref[0]["pairs"].tobytes() == ref[2]["pairs"].tobytes() and ref[0]["best"] != ref[2]["best"]   # the repeated edge: another seed
    assert ref[0]["pairs_n"] > 256 or reference(33, False, 1.0, 2000)[0]["pairs_n"] == 257   # more than one scoring tile


@pytest.mark.parametrize("H", [1, 255, 2000])
@pytest.mark.parametrize("mutual,ratio", [(False, 1.0), (True, 1.0), (False, 0.8), (True, 0.8)])
@pytest.mark.parametrize("dim", [33, 7])
def test_equals_the_single_calls_and_the_reference(eng, dim, mutual, ratio, H):
    desc, xyz, off = sets(dim)
    src, dst = [e[0] for e in EDGES], [e[1] for e in EDGES]
    want = reference(dim, mutual, ratio, H)
    loop = single_calls(eng, desc, xyz, off, EDGES, SEEDS, mutual, ratio, H, TAU, EDGE_SIM)
    for e, (a, b) in enumerate(zip(loop, want)):   # (the yardstick agrees with its own statement)
        assert all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in ("pose", "pairs", "flags")), e
        assert all(int(a[k]) == int(b[k]) for k in ("pairs_n", "best", "count", "accepted")), e
    res = eng.coarse_pairs(desc, xyz, off, src, dst, SEEDS, mutual=mutual, ratio=ratio, hypotheses=H, tau=TAU, edge_sim=EDGE_SIM)
    assert_edges(res, eng.coarse_pairs_fetch, want, (dim, mutual, ratio, H, "reference"))
    assert_edges(res, eng.coarse_pairs_fetch, loop, (dim, mutual, ratio, H, "single calls"))


@pytest.mark.parametrize("dim", [33, 7])
def test_host_and_device_pointers_give_the_same_bytes(eng, dim):
    desc, xyz, off = sets(dim)
    src, dst = [e[0] for e in EDGES], [e[1] for e in EDGES]
    want = reference(dim, True, 1.0, 255)
    dev = torch.device("cuda", 0)
    for d_dev, x_dev in ((True, True), (True, False), (False, True)):
        d = torch.from_numpy(desc).to(dev) if d_dev else desc
        x = torch.from_numpy(xyz).to(dev) if x_dev else xyz
        res = eng.coarse_pairs(d, x, off, src, dst, SEEDS, mutual=True, ratio=1.0, hypotheses=255, tau=TAU, edge_sim=EDGE_SIM)
        assert_edges(res, eng.coarse_pairs_fetch, want, (dim, d_dev, x_dev, "host fetch"))
        assert_edges(res, lambda e: eng.coarse_pairs_fetch(e, device=True), want, (dim, d_dev, x_dev, "device fetch"))


def test_default_and_integer_seeds_and_match_chunk(eng):
    desc, xyz, off = sets(33)
    edges = EDGES[:4]
    src, dst = [e[0] for e in edges], [e[1] for e in edges]
    for seed_arg, first in ((None, 0), (7, 7), (2 ** 64 - 2, 2 ** 64 - 2)):
        seeds = [(first + e) % 2 ** 64 for e in range(len(edges))]
        want = [ir.coarse_edge(rows(desc, off, a), rows(xyz, off, a), rows(desc, off, b), rows(xyz, off, b), True, 1.0, 255, s, TAU, EDGE_SIM)
                for (a, b), s in zip(edges, seeds)]
        res = eng.coarse_pairs(desc, xyz, off, src, dst, seed_arg, hypotheses=255, tau=TAU, edge_sim=EDGE_SIM)
        assert_edges(res, eng.coarse_pairs_fetch, want, ("seeds", seed_arg))
    for chunk in (1, 100, 2048):   # the option changes speed only
        eng.set_option("match_chunk", chunk)
        try:
            res = eng.coarse_pairs(desc, xyz, off, src, dst, seeds, hypotheses=255, tau=TAU, edge_sim=EDGE_SIM)
            assert_edges(res, eng.coarse_pairs_fetch, want, ("match_chunk", chunk))
        finally:
            eng.set_option("match_chunk", 64)


def test_no_edges_is_not_an_error(eng):
    desc, xyz, off = sets(7)
    res = eng.coarse_pairs(desc, xyz, off, [], [], None, hypotheses=10, tau=TAU)
    assert len(res["pairs"]) == 0 and res["pose"].shape == (0, 4, 4)
    assert eng.lib.mvicp_coarse_pairs_fetch(eng.h, 0, 0, None, None) == ERR_ARG   # (a result with no edge in it)


def test_the_chain_on_the_fixture_cut_to_300_points(eng):
    """fpfhref descriptors of the four views at 300 points each: the real chain, every edge, H = 8000"""
    cl, ref = ir.fixture_clouds(300), ir.fixture_reference(300)
    desc, xyz = np.ascontiguousarray(np.concatenate(ref["desc"])), np.ascontiguousarray(np.concatenate(cl["xyz"]))
    off = np.arange(5, dtype=np.int64) * 300
    src, dst = [e[0] for e in ir.FIX_EDGES], [e[1] for e in ir.FIX_EDGES]
    seeds = [ir.fix_seed(i, j) for i, j in ir.FIX_EDGES]
    assert any(r["best"] >= 0 and r["count"] >= 3 for r in ref["edges"])
    eng.set_option("match_chunk", 2048)
    try:
        res = eng.coarse_pairs(desc, xyz, off, src, dst, seeds, hypotheses=ir.FIX_H, tau=cl["tau"], edge_sim=ir.FIX_EDGE_SIM)
    finally:
        eng.set_option("match_chunk", 64)
    assert_edges(res, eng.coarse_pairs_fetch, ref["edges"], "fixture at 300")


# ---- state
def fetch_others(eng, m, n, H, c, rows_fpfh):
    """the last results of feature_match, consensus, fpfh and knn_search, as bytes"""
    lib, out = eng.lib, []
    fi, fd, bi, bd = np.zeros((m, 2), np.int32), np.zeros((m, 2)), np.zeros((n, 2), np.int32), np.zeros((n, 2))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mvicp_feature_match_fetch(eng.h, m, n, vp(fi), vp(fd), vp(bi), vp(bd)) == 0
    counts, flags = np.zeros(H, np.int32), np.zeros(c, np.uint8)
    assert lib.mvicp_consensus_fetch(eng.h, H, vp(counts), c, vp(flags)) == 0
    desc, used = np.zeros((rows_fpfh, 33)), np.zeros(rows_fpfh, np.int32)
    assert lib.mvicp_fpfh_fetch(eng.h, rows_fpfh, vp(desc), vp(used)) == 0
    cnt, idx, d2 = np.zeros(rows_fpfh, np.int32), np.zeros((rows_fpfh, 8), np.int32), np.zeros((rows_fpfh, 8))
    assert lib.mvicp_knn_fetch(eng.h, rows_fpfh, rows_fpfh * 8, vp(cnt), None, vp(idx), vp(d2)) == 0
    return [a.tobytes() for a in (fi, fd, bi, bd, counts, flags, desc, used, cnt, idx, d2)]


def test_the_other_results_are_left_untouched(eng):
    desc, xyz, off = sets(33)
    p, nrm = mr.bumps(200, 5)
    eng.set_frames([p], [nrm])
    eng.fpfh(0, 0.2, 8)
    a, b = rows(desc, off, 4), rows(desc, off, 5)
    eng.feature_match(a, b)
    eng.consensus(rows(xyz, off, 4)[:60], rows(xyz, off, 5)[:60], 300, 3, TAU, EDGE_SIM)
    before = fetch_others(eng, len(a), len(b), 300, 60, 200)
    src, dst = [e[0] for e in EDGES], [e[1] for e in EDGES]
    eng.coarse_pairs(desc, xyz, off, src, dst, SEEDS, hypotheses=255, tau=TAU, edge_sim=EDGE_SIM)
    assert fetch_others(eng, len(a), len(b), 300, 60, 200) == before
    with pytest.raises(mvicp.MvicpError):   # a failed call leaves them alone as well
        bad = desc.copy(); bad[5, 0] = np.inf
        eng.coarse_pairs(bad, xyz, off, src, dst, SEEDS, hypotheses=255, tau=TAU, edge_sim=EDGE_SIM)
    assert fetch_others(eng, len(a), len(b), 300, 60, 200) == before


def test_the_second_call_replaces_the_first(eng):
    desc, xyz, off = sets(33)
    src, dst = [e[0] for e in EDGES], [e[1] for e in EDGES]
    eng.coarse_pairs(desc, xyz, off, src, dst, SEEDS, hypotheses=255, tau=TAU, edge_sim=EDGE_SIM)
    d7, x7, off7 = sets(7)
    res = eng.coarse_pairs(d7, x7, off7, src[:3], dst[:3], SEEDS[:3], mutual=False, ratio=0.8, hypotheses=2000, tau=TAU, edge_sim=EDGE_SIM)
    assert_edges(res, eng.coarse_pairs_fetch, reference(7, False, 0.8, 2000)[:3], "second call")
    assert eng.lib.mvicp_coarse_pairs_fetch(eng.h, 3, 1 << 20, None, None) == ERR_ARG   # (edge 3 was the first call's)


def test_a_non_finite_input_leaves_no_result(eng):
    desc, xyz, off = sets(7)
    src, dst = [e[0] for e in EDGES], [e[1] for e in EDGES]
    for which, row in (("desc", 0), ("desc", len(desc) - 1), ("xyz", 70), ("xyz", len(xyz) - 1)):
        for value in (np.nan, -np.inf):
            eng.coarse_pairs(desc, xyz, off, src, dst, SEEDS, hypotheses=10, tau=TAU, edge_sim=EDGE_SIM)
            assert eng.lib.mvicp_coarse_pairs_fetch(eng.h, 0, 1 << 20, None, None) == 0
            d, x = desc.copy(), xyz.copy()
            (d if which == "desc" else x)[row, -1] = value
            with pytest.raises(mvicp.MvicpError, match="not finite"):
                eng.coarse_pairs(d, x, off, src, dst, SEEDS, hypotheses=10, tau=TAU, edge_sim=EDGE_SIM)
            assert eng.lib.mvicp_coarse_pairs_fetch(eng.h, 0, 1 << 20, None, None) == ERR_STATE
    # a value in a set that no edge touches is an input all the same
    d = desc.copy(); d[off[8], 0] = np.nan
    with pytest.raises(mvicp.MvicpError, match="not finite"):
        eng.coarse_pairs(d, xyz, off, [6], [7], [1], hypotheses=10, tau=TAU, edge_sim=EDGE_SIM)


def test_every_argument_error(eng):
    lib = eng.lib
    desc, xyz, off = sets(7)
    src, dst = np.array([6, 7], dtype=np.int32), np.array([7, 6], dtype=np.int32)
    seeds = np.array([1, 2], dtype=np.uint64)
    res = (L.CoarseEdge * 2)()
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))

    def call(h=eng.h, d=desc, x=xyz, o=off, n_sets=len(SET_ROWS), dim=7, E=2, s=src, t=dst, sd=seeds, ratio=1.0, H=100, tau=TAU, edge_sim=0.9, r=res):
        return lib.mvicp_coarse_pairs(h, vp(d), vp(x), None if o is None else o.ctypes.data_as(C.POINTER(C.c_longlong)), n_sets, dim, E, ip(s), ip(t),
                                      None if sd is None else sd.ctypes.data_as(C.POINTER(C.c_ulonglong)), 1, ratio, H, tau, edge_sim, r)

    assert call() == 2
    good = [eng.coarse_pairs_fetch(e) for e in range(2)]
    i32 = lambda *v: np.array(v, dtype=np.int32)
    off_dec = off.copy(); off_dec[3] = off_dec[2] - 1
    off_start = off.copy(); off_start[0] = 1
    off_big = np.array([0, 2 ** 31], dtype=np.int64)
    many = np.zeros(65536, dtype=np.int32)
    bad = (dict(h=None), dict(d=None), dict(x=None), dict(o=None), dict(s=None), dict(t=None), dict(sd=None), dict(r=None), dict(dim=0), dict(dim=65),
           dict(n_sets=0), dict(E=-1), dict(E=65536, s=many, t=many + 1, sd=np.zeros(65536, np.uint64), H=1), dict(s=i32(6, 9)), dict(t=i32(7, -1)),
           dict(s=i32(6, 6), t=i32(7, 6)), dict(o=off_dec), dict(o=off_start), dict(o=off_big, n_sets=1, E=0), dict(H=0), dict(H=2 ** 24 + 1),
           dict(E=17, s=many[:17] + 6, t=many[:17] + 7, sd=np.zeros(17, np.uint64), r=(L.CoarseEdge * 17)(), H=2 ** 24), dict(ratio=float("nan")), dict(ratio=0.0), dict(ratio=-1.0), dict(tau=0.0), dict(tau=float("inf")), dict(tau=float("nan")),
           dict(edge_sim=1.0), dict(edge_sim=-0.1), dict(edge_sim=float("nan")))
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
        assert lib.mvicp_last_error()
    # decided before the context was touched: the last result is still there
    for e in range(2):
        pr, fl = eng.coarse_pairs_fetch(e)
        assert pr.tobytes() == good[e][0].tobytes() and fl.tobytes() == good[e][1].tobytes()
    # the fetch
    c = len(good[0][0])
    buf, fl = np.zeros((c, 2), np.int32), np.zeros(c, np.uint8)
    assert c > 0 and lib.mvicp_coarse_pairs_fetch(eng.h, 0, c, vp(buf), vp(fl)) == 0
    assert lib.mvicp_coarse_pairs_fetch(None, 0, c, vp(buf), vp(fl)) == ERR_ARG
    assert lib.mvicp_coarse_pairs_fetch(eng.h, 0, c - 1, vp(buf), vp(fl)) == ERR_ARG
    assert lib.mvicp_coarse_pairs_fetch(eng.h, -1, c, vp(buf), vp(fl)) == ERR_ARG
    assert lib.mvicp_coarse_pairs_fetch(eng.h, 2, c, vp(buf), vp(fl)) == ERR_ARG
    fresh = mvicp.Engine(0)
    try:
        assert lib.mvicp_coarse_pairs_fetch(fresh.h, 0, c, vp(buf), vp(fl)) == ERR_STATE
    finally:
        fresh.close()


# ---- the clouds-alone initialisation
def test_init_from_clouds_equals_the_cpu_chain(eng):
    """GPU FPFH descriptors are the bytes of fpfhref's, so the whole initialisation is: with refine off the poses equal the CPU chain's byte
    for byte, with refine on the tree is the same (the counts decide it) and each refined tree edge stays within the 3 deg / 3 spacings of
    tests/test_match_cpu.py of the truth."""
    cl, ref = ir.fixture_clouds(), ir.fixture_reference()
    eng.set_frames(cl["xyz"], cl["nrm"])
    eng.set_option("match_chunk", 2048)
    try:
        seeds_ok = [ir.fix_seed(i, j) for i, j in ir.FIX_EDGES] != [12345 + e for e in range(6)]
        assert seeds_ok   # (the fixture's seeds are not seed + e: init_from_clouds is checked through its counts at seed = 12345 below)
        for refine in (False, True):
            out = init_with_fixture_seeds(eng, cl, refine)
            for e, (rec, want) in enumerate(zip(out["records"], ref["edges"])):
                assert (rec["pairs"], rec["accepted"], rec["inliers"], rec["best"]) == (want["pairs_n"], want["accepted"], want["count"], want["best"]), e
                assert rec["pose"].tobytes() == want["pose"].tobytes(), e
            for key in ("parent", "parent_edge", "component"):
                assert out[key].tobytes() == ref["tree"][key].tobytes(), (refine, key)
            assert out["components"] == 1
            if not refine:
                assert out["poses"].tobytes() == ref["tree"]["poses"].tobytes()
            else:
                for k in range(1, 4):
                    i, j = ir.FIX_EDGES[out["parent_edge"][k]]
                    deg, dt = ir.pose_error(out["records"][out["parent_edge"][k]]["refined"], ir.relative_truth(cl["gt"], i, j))
                    print("refined edge", (i, j), deg, dt / cl["spacing"])
                    assert deg < 3.0 and dt < 3.0 * cl["spacing"]
    finally:
        eng.set_option("match_chunk", 64)


def init_with_fixture_seeds(eng, cl, refine):
    """mvicp.init_from_clouds draws seeds[e] = seed + e; the fixture's are 12345 + 4 i + j.  Each edge list below is a run of edges whose
    fixture seeds ascend by one, so the public function is called as it is and the pieces are joined by poses_from_pairs."""
    runs = (((0, 1), (0, 2), (0, 3)), ((1, 2), (1, 3)), ((2, 3),))
    records = []
    for run in runs:
        part = mvicp.init_from_clouds(eng, [0, 1, 2, 3], cl["xyz"], cl["radius"], cl["tau"], max_nn=ir.FIX_MAX_NN, edges=run, hypotheses=ir.FIX_H,
                                      seed=ir.fix_seed(*run[0]), edge_sim=ir.FIX_EDGE_SIM, min_count=ir.FIX_MIN_COUNT, refine=refine)
        assert [tuple(e) for e in part["edges"].tolist()] == list(run)
        records += part["records"]
    src, dst = [e[0] for e in ir.FIX_EDGES], [e[1] for e in ir.FIX_EDGES]
    tree = mvicp.poses_from_pairs(4, src, dst, [r["inliers"] for r in records], np.array([r["refined"] if refine else r["pose"] for r in records]),
                                  ir.FIX_MIN_COUNT, 0)
    tree["records"] = records
    return tree


def test_init_from_clouds_in_one_call(eng):
    """all i < j edges by default, seeds seed + e: the same as coarse_pairs on the CPU's descriptors with those seeds, and the tree that
    poses_from_pairs builds from its counts"""
    cl, ref = ir.fixture_clouds(300), ir.fixture_reference(300)
    eng.set_frames(cl["xyz"], cl["nrm"])
    out = mvicp.init_from_clouds(eng, [0, 1, 2, 3], cl["xyz"], cl["radius"], cl["tau"], hypotheses=500, seed=77, min_count=3, refine=False)
    assert [tuple(e) for e in out["edges"].tolist()] == list(ir.FIX_EDGES)
    want = [ir.coarse_edge(ref["desc"][i], cl["xyz"][i], ref["desc"][j], cl["xyz"][j], True, 1.0, 500, 77 + e, cl["tau"], 0.9) for e, (i, j) in enumerate(ir.FIX_EDGES)]
    for rec, w in zip(out["records"], want):
        assert (rec["pairs"], rec["accepted"], rec["inliers"], rec["best"]) == (w["pairs_n"], w["accepted"], w["count"], w["best"])
        assert rec["pose"].tobytes() == w["pose"].tobytes()
    tree = ir.poses_from_pairs(4, [e[0] for e in ir.FIX_EDGES], [e[1] for e in ir.FIX_EDGES], [w["count"] for w in want], np.array([w["pose"] for w in want]), 3, 0)
    for key in ("poses", "parent", "parent_edge", "component"):
        assert out[key].tobytes() == tree[key].tobytes(), key
