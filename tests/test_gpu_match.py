"""mvicp_feature_match / mvicp_consensus (and mvicp.coarse_align on top of them) on the MI355X: every result equals the numpy statement
of the contract (tests/matchref.py) byte for byte; no tolerance anywhere.  What a case must contain (exact ties, padding, several
chunks, rejected hypotheses, a distance equal to tau2, ties in the count) is asserted on the reference alone, so no case can pass
trivially."""
import ctypes as C

import numpy as np
import pytest

import matchref as mr
import mvicp
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3


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


def descriptors(m, n, dim, seed, integer=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    if integer:   # small integers and duplicated rows: exact ties, first and second place alike
        a, b = rng.integers(0, 3, size=(m, dim)).astype(np.float64), rng.integers(0, 3, size=(n, dim)).astype(np.float64)
        b[n // 2:] = b[:n - n // 2]
        return a, b
    return rng.uniform(0.0, 100.0, size=(m, dim)), rng.uniform(0.0, 100.0, size=(n, dim))


# ---- matching
@pytest.mark.parametrize("dim", [1, 33, 64])
@pytest.mark.parametrize("shape", [(130, 257), (1, 1), (5, 1), (0, 9), (9, 0)])
def test_match_shapes(eng, dim, shape):
    a, b = descriptors(*shape, dim, 100 + dim)
    want = mr.feature_match(a, b)
    if shape == (5, 1):
        assert (want["fwd_idx"][:, 1] == -1).all() and np.isinf(want["fwd_d2"][:, 1]).all()
    assert_match(eng.feature_match(a, b), want, (shape, dim))
    assert_match(eng.feature_match(a, b, device=True), want, (shape, dim, "device destinations"))


@pytest.mark.parametrize("dim", [1, 33, 64])
def test_match_ties_and_chunks(eng, dim):
    a, b = descriptors(130, 257, dim, 7, integer=True)
    want = mr.feature_match(a, b)
    tie = want["fwd_d2"][:, 0] == want["fwd_d2"][:, 1]
    assert tie.sum() > 60 and (want["fwd_idx"][tie, 0] < want["fwd_idx"][tie, 1]).all()
    if dim > 1:   # a tie that spans two chunks of 64: the duplicate of row j is row j + 128
        assert (want["fwd_idx"][tie, 1] // 64 != want["fwd_idx"][tie, 0] // 64).sum() > 30
    assert_match(eng.feature_match(a, b), want, ("ties", dim))
    try:
        eng.set_option("match_chunk", 64)     # five chunks at n = 257, three at m = 130: the merge runs
        assert_match(eng.feature_match(a, b), want, ("ties, chunks of 64", dim))
        c, d = descriptors(130, 257, dim, 8)
        assert_match(eng.feature_match(c, d), mr.feature_match(c, d), ("chunks of 64", dim))
        eng.set_option("match_chunk", 1)
        assert_match(eng.feature_match(a[:9], b[:70]), mr.feature_match(a[:9], b[:70]), ("chunks of 1", dim))
    finally:
        eng.set_option("match_chunk", 2048)


def test_match_fpfh_descriptors_on_the_device(eng):
    cl, ref = mr.e2e_clouds(False), mr.e2e_reference(False)
    eng.set_frames([cl["src"], cl["dst"]], [cl["src_nrm"], cl["dst_nrm"]])
    da = eng.fpfh(0, cl["radius"], mr.E2E_MAX_NN, device=True)["desc"]
    db = eng.fpfh(1, cl["radius"], mr.E2E_MAX_NN, device=True)["desc"]
    assert da.is_cuda and da.cpu().numpy().tobytes() == ref["desc_src"].tobytes() and db.cpu().numpy().tobytes() == ref["desc_dst"].tobytes()
    got = eng.feature_match(da, db, device=True)
    assert all(v.is_cuda for v in got.values())
    assert_match(got, ref["match"], "fpfh, device pointers")
    assert_match(eng.feature_match(da, ref["desc_dst"]), ref["match"], "fpfh, one device and one host operand")
    got = host(got)
    for mutual in (True, False):
        for ratio in (1.0, 0.8):
            want = mr.match_pairs(ref["match"]["fwd_idx"], ref["match"]["fwd_d2"], ref["match"]["bwd_idx"], mutual, ratio)
            pairs = mvicp.match_pairs(got["fwd_idx"], got["fwd_d2"], got["bwd_idx"], mutual, ratio)
            assert len(want) > 100 and pairs.dtype == np.int32 and pairs.tobytes() == want.tobytes(), (mutual, ratio)


# ---- consensus
def test_consensus_end_to_end_pairs(eng):
    cl, ref = mr.e2e_clouds(False), mr.e2e_reference(False)
    P, Q, want = ref["P"], ref["Q"], ref["consensus"]
    assert len(P) % 64 != 0 and len(P) > 256 and want["accepted"] % 256 != 0 and want["best"] >= 0
    assert_consensus(eng.consensus(P, Q, mr.E2E_H, mr.E2E_SEED, cl["tau"], mr.E2E_EDGE_SIM), want, "end to end")
    dev = torch.device("cuda", 0)
    got = eng.consensus(torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev), mr.E2E_H, mr.E2E_SEED, cl["tau"], mr.E2E_EDGE_SIM)
    assert_consensus(got, want, "end to end, device pointers")
    for seed in (1, 2 ** 64 - 1):
        w = mr.consensus(P, Q, 3000, seed, cl["tau"], mr.E2E_EDGE_SIM)
        assert w["accepted"] > 50 and w["best"] != want["best"]
        assert_consensus(eng.consensus(P, Q, 3000, seed, cl["tau"], mr.E2E_EDGE_SIM), w, ("seed", seed))
    w = mr.consensus(P, Q, 1000, 5, cl["tau"], 0.0)
    assert w["accepted"] > 900                       # edge_sim = 0: only repeated indices reject
    assert_consensus(eng.consensus(P, Q, 1000, 5, cl["tau"], 0.0), w, "edge_sim 0")


def test_consensus_smallest_cases(eng):
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    Q = np.ascontiguousarray(P[:, [1, 2, 0]] + 1.0)
    w = mr.consensus(P, Q, 64, 9, 0.5, 0.9)             # c = 3
    assert 0 < w["accepted"] < 64 and w["count"] == 3
    assert_consensus(eng.consensus(P, Q, 64, 9, 0.5, 0.9), w, "c = 3")
    seen = set()
    for seed in range(6):                                # H = 1, accepted or not
        w = mr.consensus(P, Q, 1, seed, 0.5, 0.9)
        seen.add(w["best"])
        assert_consensus(eng.consensus(P, Q, 1, seed, 0.5, 0.9), w, ("H = 1", seed))
    assert seen == {-1, 0}


def test_consensus_lattice_inclusive_bound_and_ties(eng):
    rng = np.random.Generator(np.random.PCG64(21))
    lat = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    P = np.ascontiguousarray(lat[rng.permutation(len(lat))])
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Q = np.ascontiguousarray(P @ Rz.T + np.array([2.0, -3.0, 5.0]))
    Q[::3] += rng.integers(-1, 2, size=(len(Q[::3]), 3))          # a third of the pairs moved by lattice steps: residuals are integers
    tau = 1.0                                                      # tau2 = 1 is a squared distance that occurs
    w = mr.consensus(P, Q, 2000, 4, tau, 0.9)
    ok, R, t, _ = mr.hypotheses(P, Q, 2000, 4, 0.9)
    exact = np.flatnonzero(ok & (np.abs(R - Rz).max((1, 2)) == 0) & (np.abs(t - [2.0, -3.0, 5.0]).max(1) == 0))
    assert len(exact) > 5                                          # hypotheses that are the exact rotation: their residuals are exact integers
    r2 = (((P @ Rz.T + [2.0, -3.0, 5.0]) - Q) ** 2).sum(1)
    assert (r2 == 1.0).sum() > 5 and w["count"] == (r2 <= 1.0).sum() and w["count"] > (r2 < 1.0).sum()   # the inclusive <=
    assert (w["counts"] == w["count"]).sum() > 1 and w["best"] == np.flatnonzero(w["counts"] == w["count"])[0]   # the lowest h among equals
    assert_consensus(eng.consensus(P, Q, 2000, 4, tau, 0.9), w, "lattice")


def test_consensus_collinear(eng):
    P = np.outer(np.arange(20.0), [1.0, 2.0, -1.0])
    w = mr.consensus(P, P.copy(), 500, 3, 1.0, 0.0)
    assert w["best"] == -1 and w["accepted"] == 0
    got = eng.consensus(P, P.copy(), 500, 3, 1.0, 0.0)
    assert_consensus(got, w, "collinear")
    assert got["pose"].tobytes() == np.eye(4).tobytes() and got["count"] == 0 and (got["counts"] == -1).all() and not got["flags"].any()


# ---- the helper
@pytest.mark.parametrize("partial", [False, True])
def test_coarse_align(eng, partial):
    cl, ref = mr.e2e_clouds(partial), mr.e2e_reference(partial)
    eng.set_frames([cl["src"], cl["dst"]], [cl["src_nrm"], cl["dst_nrm"]])
    got = mvicp.coarse_align(eng, 0, 1, cl["src"], cl["dst"], cl["radius"], mr.E2E_MAX_NN, hypotheses=mr.E2E_H, seed=mr.E2E_SEED, tau=cl["tau"],
                             edge_sim=mr.E2E_EDGE_SIM, mutual=True, ratio=1.0)
    want = ref["consensus"]
    assert got["pairs"].tobytes() == ref["pairs"].tobytes()
    assert got["pose"].tobytes() == want["pose"].tobytes() and got["inliers"].tobytes() == want["flags"].tobytes()
    assert got["counts"] == {"pairs": len(ref["pairs"]), "accepted": want["accepted"], "inliers": want["count"], "best": want["best"]}
    keep = want["flags"] != 0
    refined = mvicp.lib.closedform_point_to_point(ref["P"][keep], ref["Q"][keep])
    assert got["refined"].tobytes() == refined.tobytes()
    deg, dt = mr.pose_error(got["pose"], cl["truth"])
    assert deg < 3.0 and dt < 3.0 * cl["spacing"]


# ---- errors and state
def test_errors_and_state():
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        a, b = descriptors(20, 30, 33, 1)
        fi, fd, bi, bd = np.zeros((20, 2), np.int32), np.zeros((20, 2)), np.zeros((30, 2), np.int32), np.zeros((30, 2))
        assert lib.mvicp_feature_match_fetch(h, 20, 30, vp(fi), vp(fd), vp(bi), vp(bd)) == ERR_STATE and b"mvicp_feature_match first" in lib.mvicp_last_error()
        assert lib.mvicp_consensus_fetch(h, 10, None, 10, None) == ERR_STATE and b"mvicp_consensus first" in lib.mvicp_last_error()
        assert lib.mvicp_feature_match(None, vp(a), 20, vp(b), 30, 33) == ERR_ARG
        assert lib.mvicp_feature_match(h, vp(a), 20, vp(b), 30, 33) == 20
        assert lib.mvicp_feature_match_fetch(h, 20, 30, vp(fi), vp(fd), vp(bi), vp(bd)) == 0
        want = mr.feature_match(a, b)
        assert_match({"fwd_idx": fi, "fwd_d2": fd, "bwd_idx": bi, "bwd_d2": bd}, want, "20 x 30")
        assert lib.mvicp_feature_match_fetch(h, 19, 30, vp(fi), None, None, None) == ERR_ARG and b"cap_m" in lib.mvicp_last_error()
        assert lib.mvicp_feature_match_fetch(h, 20, 29, None, None, None, vp(bd)) == ERR_ARG and b"cap_n" in lib.mvicp_last_error()
        assert lib.mvicp_feature_match_fetch(h, 0, 30, None, None, vp(bi), None) == 0              # only one of the destinations
        # an argument error leaves the last result alone
        for args in ((vp(a), 20, vp(b), 30, 0), (vp(a), 20, vp(b), 30, 65), (vp(a), -1, vp(b), 30, 33), (vp(a), 20, vp(b), 1 << 31, 33), (None, 20, vp(b), 30, 33)):
            assert lib.mvicp_feature_match(h, *args) == ERR_ARG, args
        fd2 = np.zeros((20, 2))
        assert lib.mvicp_feature_match_fetch(h, 20, 30, None, vp(fd2), None, None) == 0 and fd2.tobytes() == want["fwd_d2"].tobytes()
        # a non-finite value is reported by the call, and no result is left behind
        for bad in (np.nan, np.inf):
            assert lib.mvicp_feature_match(h, vp(a), 20, vp(b), 30, 33) == 20
            c = b.copy(); c[29, 32] = bad
            assert lib.mvicp_feature_match(h, vp(a), 20, vp(c), 30, 33) == ERR_ARG and b"finite" in lib.mvicp_last_error()
            assert lib.mvicp_feature_match_fetch(h, 20, 30, None, vp(fd2), None, None) == ERR_STATE
        assert lib.mvicp_set_option(h, b"match_chunk", C.c_double(0.0)) == ERR_ARG
        # consensus
        P, Q = np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(a[:, 3:6])
        res = mvicp.lib.ConsensusResult()
        ok = (vp(P), vp(Q), 20, 100, 7, 30.0, 0.5, C.byref(res))
        assert lib.mvicp_consensus(h, *ok) == 0
        counts, flags = np.zeros(100, np.int32), np.zeros(20, np.uint8)
        assert lib.mvicp_consensus_fetch(h, 100, vp(counts), 20, vp(flags)) == 0
        w = mr.consensus(P, Q, 100, 7, 30.0, 0.5)
        assert w["accepted"] > 0 and counts.tobytes() == w["counts"].tobytes() and flags.tobytes() == w["flags"].tobytes() and res.best == w["best"]
        assert lib.mvicp_consensus_fetch(h, 99, vp(counts), 20, None) == ERR_ARG and b"cap_h" in lib.mvicp_last_error()
        assert lib.mvicp_consensus_fetch(h, 100, None, 19, vp(flags)) == ERR_ARG and b"cap_c" in lib.mvicp_last_error()
        nan, inf = float("nan"), float("inf")
        for args in ((vp(P), vp(Q), 2, 100, 7, 30.0, 0.5), (vp(P), vp(Q), 20, 0, 7, 30.0, 0.5), (vp(P), vp(Q), 20, (1 << 24) + 1, 7, 30.0, 0.5),
                     (vp(P), vp(Q), 20, 100, 7, 0.0, 0.5), (vp(P), vp(Q), 20, 100, 7, nan, 0.5), (vp(P), vp(Q), 20, 100, 7, inf, 0.5),
                     (vp(P), vp(Q), 20, 100, 7, 30.0, 1.0), (vp(P), vp(Q), 20, 100, 7, 30.0, -0.1), (vp(P), vp(Q), 20, 100, 7, 30.0, nan),
                     (None, vp(Q), 20, 100, 7, 30.0, 0.5), (vp(P), None, 20, 100, 7, 30.0, 0.5)):
            assert lib.mvicp_consensus(h, *args, C.byref(res)) == ERR_ARG, args[2:]
        assert lib.mvicp_consensus(None, *ok) == ERR_ARG
        counts2 = np.zeros(100, np.int32)
        assert lib.mvicp_consensus_fetch(h, 100, vp(counts2), 20, None) == 0 and counts2.tobytes() == counts.tobytes()   # the last result stayed
        Pbad = P.copy(); Pbad[19, 2] = np.inf
        assert lib.mvicp_consensus(h, vp(Pbad), vp(Q), 20, 100, 7, 30.0, 0.5, C.byref(res)) == ERR_ARG and b"finite" in lib.mvicp_last_error()
        assert lib.mvicp_consensus_fetch(h, 100, vp(counts2), 20, None) == ERR_STATE
        # the results end with the frames
        assert lib.mvicp_feature_match(h, vp(a), 20, vp(b), 30, 33) == 20 and lib.mvicp_consensus(h, *ok) == 0
        assert lib.mvicp_set_num_frames(h, 1) == 0
        assert lib.mvicp_feature_match_fetch(h, 20, 30, None, None, None, None) == ERR_STATE
        assert lib.mvicp_consensus_fetch(h, 100, None, 20, None) == ERR_STATE
    finally:
        fresh.close()


def test_history_neutral():
    pb = synth.make_problem(4, 3000)
    a, b = descriptors(300, 400, 33, 2)
    P, Q = np.ascontiguousarray(a[:, :3]), np.ascontiguousarray(b[:300, :3])

    def run(with_calls):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_calls:
                e.feature_match(a, b)   # before the graph exists
                e.consensus(P, Q, 500, 1, 20.0, 0.5)
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_calls:
                    e.feature_match(a, b, device=(r == 1))
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_calls:
                    e.consensus(P, Q, 500, r, 20.0, 0.5)
                triples, offsets = e.map_correspondences()
                epochs = e.correspondence_epochs()
                blocks = e.linearize(poses, True, True)
                if with_calls:
                    e.feature_match(b, a)
                poses, sm = e.optimize(poses, pb["fixed"])
                if with_calls:
                    e.consensus(Q, P, 200, r, 10.0, 0.0)   # between rounds
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            epochs.tobytes(), sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)
