"""The size-selected kernel paths of mvicp_consensus and mvicp_feature_match on the MI355X: the cases of tests/pathcases.py, each compared
with the numpy statement of the contract (tests/matchref.py) byte for byte; no tolerance anywhere.  Every case first asserts, on the launch
plan and the reference alone, that it reaches the branch it is built for (tests/test_paths_cpu.py does the same without a GPU); the
profile's model bytes, from which the launched grid can be recovered, are held against the plan."""
import numpy as np
import pytest

import matchref as mr
import mvicp
import pathcases as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def host(d):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def assert_match(got, want, what):
    got = host(got)
    for key in mr.MATCH_KEYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            raise AssertionError((what, key, len(bad), bad[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), b.reshape(-1)[bad[:4]].tolist()))


def assert_consensus(got, want, what):
    for key in ("best", "count", "accepted"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert got["pose"].tobytes() == want["pose"].tobytes(), (what, "pose", got["pose"], want["pose"])
    assert got["counts"].dtype == np.int32 and got["counts"].tobytes() == want["counts"].tobytes(), (what, "counts", np.flatnonzero(got["counts"] != want["counts"])[:8])
    assert got["flags"].dtype == np.uint8 and got["flags"].tobytes() == want["flags"].tobytes(), (what, "flags")


def profiled(eng, scope, call):
    """-> (the result of call(), the model bytes booked on `scope` by it)"""
    eng.profile(True)
    try:
        eng.profile_reset()
        got = call()
        rec = eng.profile_get_ex(scope)
    finally:
        eng.profile(False)
    assert rec["launches"] == 1, (scope, rec)
    return got, rec["model_bytes"]


# ---- consensus
def run_consensus(eng, name, device=False):
    P, Q, H = pc.consensus_pairs(name)
    if device:
        dev = torch.device("cuda", 0)
        P, Q = torch.from_numpy(np.array(P)).to(dev), torch.from_numpy(np.array(Q)).to(dev)
    return eng.consensus(P, Q, H, pc.CONS_SEED, pc.CONS_TAU, pc.CONS_EDGE_SIM)


def test_c1_many_pairs_and_few_hypotheses(eng):
    """gx = 1 and more tiles than workgroup rows: every workgroup re-stages its LDS tile once (the barrier at the head of the loop is
    needed), and the last workgroup row holds a single pair."""
    plan, want = pc.check_consensus_case("C1")
    c = len(pc.consensus_pairs("C1")[0])
    got, model_bytes = profiled(eng, "cons_score", lambda: run_consensus(eng, "C1"))
    print("C1 planned", plan, "gx from the profile", pc.consensus_gx_from_bytes(model_bytes, c, want["accepted"]))
    assert_consensus(got, want, "C1, host arrays")
    assert pc.consensus_gx_from_bytes(model_bytes, c, got["accepted"]) == plan["gx"]
    assert_consensus(run_consensus(eng, "C1", device=True), want, "C1, device tensors")


def test_c2_many_accepted_hypotheses(eng):
    """more than 512 workgroup columns: two workgroup rows, the first walks two tiles and the second one partial tile."""
    plan, want = pc.check_consensus_case("C2")
    c = len(pc.consensus_pairs("C2")[0])
    got, model_bytes = profiled(eng, "cons_score", lambda: run_consensus(eng, "C2"))
    print("C2 planned", plan, "gx from the profile", pc.consensus_gx_from_bytes(model_bytes, c, want["accepted"]))
    assert_consensus(got, want, "C2")
    assert pc.consensus_gx_from_bytes(model_bytes, c, got["accepted"]) == plan["gx"]


def test_c3_one_full_tile_plus_one_pair(eng):
    pc.check_consensus_case("C3")
    assert_consensus(run_consensus(eng, "C3"), pc.consensus_reference("C3"), "C3")


def test_c4_georeferenced_pairs(eng):
    _, want = pc.check_consensus_case("C4")
    assert_consensus(run_consensus(eng, "C4"), want, "C4, host arrays")
    assert_consensus(run_consensus(eng, "C4", device=True), want, "C4, device tensors")


# ---- matching
def run_match(eng, name, dim, chunk, device=False):
    a, b = pc.MATCH_BUILDERS[name](dim)
    try:
        eng.set_option("match_chunk", chunk)
        return eng.feature_match(a, b, device=device)
    finally:
        eng.set_option("match_chunk", pc.MATCH_DEFAULT_CHUNK)


@pytest.mark.parametrize("dim", pc.MATCH_DIMS)
def test_m1_the_chunk_count_clamp(eng, dim):
    fwd, bwd, want = pc.check_match_case("M1", dim, 1)
    a, b = pc.match_m1(dim)
    got, model_bytes = profiled(eng, "match_fwd", lambda: run_match(eng, "M1", dim, 1))
    chunks = pc.match_chunks_from_bytes(model_bytes, fwd["wgs"], len(a), len(b), dim)
    print("M1", dim, "planned", fwd, "chunks from the profile", chunks)
    assert_match(got, want, ("M1", dim))
    assert chunks == fwd["chunks"]


@pytest.mark.parametrize("dim", pc.MATCH_DIMS)
def test_m2_chunks_that_end_inside_a_tile(eng, dim):
    fwd, bwd, want = pc.check_match_case("M2", dim, pc.M2_CHUNK)
    a, b = pc.match_m2(dim)
    got, model_bytes = profiled(eng, "match_fwd", lambda: run_match(eng, "M2", dim, pc.M2_CHUNK))
    chunks = pc.match_chunks_from_bytes(model_bytes, fwd["wgs"], len(a), len(b), dim)
    print("M2", dim, "planned", fwd, "chunks from the profile", chunks)
    assert_match(got, want, ("M2", dim))
    assert chunks == fwd["chunks"]
    assert_match(run_match(eng, "M2", dim, pc.M2_CHUNK, device=True), want, ("M2, device destinations", dim))


@pytest.mark.parametrize("order", ["a", "b", "c"])
def test_m3_the_early_exit(eng, order):
    """(a) a whole wave agrees to skip after the first segment while the next wave is kept from it by one lane, whose nearest row is among
    the skipped ones; (b) the near rows arrive last; (c) the skip comes after the second segment, not the first."""
    _, _, want = pc.check_match_case("M3" + order, 33)
    assert_match(run_match(eng, "M3" + order, 33, pc.MATCH_DEFAULT_CHUNK), want, ("M3", order))
    assert_match(run_match(eng, "M3" + order, 33, 64), want, ("M3, chunks of one tile", order))


@pytest.mark.parametrize("dim", pc.MATCH_DIMS)
def test_m4_squares_that_overflow(eng, dim):
    for chunk in (pc.MATCH_DEFAULT_CHUNK, 64):
        _, _, want = pc.check_match_case("M4", dim, chunk)
        assert_match(run_match(eng, "M4", dim, chunk), want, ("M4", dim, chunk))
