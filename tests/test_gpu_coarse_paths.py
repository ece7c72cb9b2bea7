"""-m gpu: the size-selected paths of mvicp_coarse_pairs that tests/test_gpu_coarse.py does not reach (tests/pathcases_coarse.py states
them): the chunk count clamped at kMaxChunks, the chunk cut to a short right operand, and a scoring record that walks every tile of its
edge.  Every result equals the loop of today's single-pair calls byte for byte, and the profile's model bytes, which count the work
records, are held against the plan."""
import numpy as np
import pytest

import initref as ir
import mvicp
import pathcases_coarse as pcc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
TAU = 0.05


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def profiled(eng, scopes, call):
    eng.profile(True)
    try:
        eng.profile_reset()
        out = call()
        return out, {s: eng.profile_get_ex(s) for s in scopes}
    finally:
        eng.profile(False)


def rows(arr, off, s):
    return np.ascontiguousarray(arr[off[s]:off[s + 1]])


def single_call(eng, desc, xyz, off, a, b, mutual, H, seed, edge_sim):
    mt = eng.feature_match(rows(desc, off, a), rows(desc, off, b))
    pairs = mvicp.match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, 1.0)
    rec = {"pairs_n": len(pairs), "best": -1, "count": 0, "accepted": 0, "pose": np.eye(4), "pairs": pairs, "flags": np.zeros(len(pairs), dtype=np.uint8)}
    if len(pairs) >= 3:
        cons = eng.consensus(np.ascontiguousarray(rows(xyz, off, a)[pairs[:, 0]]), np.ascontiguousarray(rows(xyz, off, b)[pairs[:, 1]]), H, seed, TAU, edge_sim)
        rec.update(best=cons["best"], count=cons["count"], accepted=cons["accepted"], pose=cons["pose"], flags=cons["flags"])
    return rec


def assert_edge(eng, res, e, want, what):
    for key, ref_key in (("pairs", "pairs_n"), ("best", "best"), ("count", "count"), ("accepted", "accepted")):
        assert int(res[key][e]) == int(want[ref_key]), (what, e, key, int(res[key][e]), want[ref_key])
    assert res["pose"][e].tobytes() == np.ascontiguousarray(want["pose"]).tobytes(), (what, e)
    pairs, flags = eng.coarse_pairs_fetch(e)
    assert pairs.tobytes() == want["pairs"].tobytes() and flags.tobytes() == want["flags"].tobytes(), (what, e)


def test_p1_the_chunk_count_is_clamped(eng):
    desc, xyz, off = pcc.p1_sets()
    m, n = pcc.P1_ROWS
    eng.set_option("match_chunk", pcc.P1_CHUNK)
    try:
        want = [single_call(eng, desc, xyz, off, 0, 1, True, 50, 5, 0.9), single_call(eng, desc, xyz, off, 1, 0, True, 50, 6, 0.9)]
        cpu = ir.coarse_edge(rows(desc, off, 0), rows(xyz, off, 0), rows(desc, off, 1), rows(xyz, off, 1), True, 1.0, 50, 5, TAU, 0.9)
        res, prof = profiled(eng, ("coarse_match",), lambda: eng.coarse_pairs(desc, xyz, off, [0, 1], [1, 0], [5, 6], hypotheses=50, tau=TAU))
    finally:
        eng.set_option("match_chunk", 2048)
    for e in range(2):
        assert_edge(eng, res, e, want[e], "P1")
    assert_edge(eng, res, 0, cpu, "P1 against the reference")
    model, records = pcc.match_model_bytes(pcc.P1_CHUNK, pcc.tables_of(pcc.P1_ROWS, [(0, 1), (1, 0)], True), pcc.P1_DIM)
    print("P1 planned records", records, "model bytes", model, "booked", prof["coarse_match"]["model_bytes"])
    assert pcc.table_plan(pcc.P1_CHUNK, m, n, pcc.P1_DIM)["clamped"]
    assert prof["coarse_match"]["launches"] == 1 and abs(prof["coarse_match"]["model_bytes"] - model) <= 1e-9 * model


@pytest.mark.parametrize("dim", [33, 7])
def test_p2_the_chunk_is_cut_to_the_right_operand(eng, dim):
    rng = np.random.Generator(np.random.PCG64(40 + dim))
    a, b = pcc.P2_ROWS
    desc = rng.integers(0, 3, size=(a + b, dim)).astype(np.float64)
    xyz = rng.uniform(0.0, 1.0, size=(a + b, 3))
    off = np.array([0, a, a + b, a + b], dtype=np.int64)   # (and a third, empty set)
    edges = [(0, 1), (1, 0), (0, 2)]
    want = [ir.coarse_edge(rows(desc, off, s), rows(xyz, off, s), rows(desc, off, d), rows(xyz, off, d), True, 1.0, 100, 9 + e, TAU, 0.9) for e, (s, d) in enumerate(edges)]
    res, prof = profiled(eng, ("coarse_match", "coarse_merge"), lambda: eng.coarse_pairs(desc, xyz, off, [e[0] for e in edges], [e[1] for e in edges], 9, hypotheses=100, tau=TAU))
    for e in range(len(edges)):
        assert_edge(eng, res, e, want[e], ("P2", dim))
    model, records = pcc.match_model_bytes(pcc.P2_CHUNK, pcc.tables_of((a, b, 0), edges, True), dim)
    print("P2", dim, "planned records", records, "booked", prof["coarse_match"]["model_bytes"])
    assert pcc.table_plan(pcc.P2_CHUNK, a, b, dim)["cut"]
    assert prof["coarse_match"]["launches"] == 1 and prof["coarse_merge"]["launches"] == 1
    assert abs(prof["coarse_match"]["model_bytes"] - model) <= 1e-9 * model


def test_p3_a_scoring_record_walks_every_tile(eng):
    desc, xyz, off = pcc.p3_sets()
    seeds = [101, 102, 103][:pcc.P3_EDGES]
    want = [single_call(eng, desc, xyz, off, 0, 1, False, pcc.P3_H, s, 0.0) for s in seeds]
    assert all(w["pairs_n"] == pcc.P3_ROWS[0] and w["count"] > 100 for w in want)
    res, prof = profiled(eng, ("coarse_score",), lambda: eng.coarse_pairs(desc, xyz, off, [0] * len(seeds), [1] * len(seeds), seeds, mutual=False,
                                                                             hypotheses=pcc.P3_H, tau=TAU, edge_sim=0.0))
    for e in range(len(seeds)):
        assert_edge(eng, res, e, want[e], "P3")
    pairs, accepted = [w["pairs_n"] for w in want], [w["accepted"] for w in want]
    plan = pcc.score_plan(pairs, accepted)
    print("P3 plan", plan["slot_blocks"], plan["want"], plan["records"], "booked", prof["coarse_score"]["model_bytes"])
    assert plan["want"] == 1 and all(e["tiles_per_record"] == 2 for e in plan["edges"])
    model = pcc.score_model_bytes(plan, pairs, accepted)
    assert prof["coarse_score"]["launches"] == 1 and abs(prof["coarse_score"]["model_bytes"] - model) <= 1e-9 * model
