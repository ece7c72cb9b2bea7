"""tests/matchref.py, the statement of mvicp_feature_match / mvicp_match_pairs / mvicp_consensus that the GPU tests compare against byte
for byte: its numpy forms equal its scalar-loop forms, the sampler and the poses have the properties the contract promises, and the
chain FPFH -> match -> pairs -> consensus finds the pose of a surface sampled twice.  Nothing here runs on a GPU; mvicp_match_pairs is a
host function and is checked here too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import matchref as mr
import mvicp
from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def descriptors(m, n, dim, seed, integer=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    if integer:   # small integers and duplicated rows: exact ties, first and second place alike
        a, b = rng.integers(0, 3, size=(m, dim)).astype(np.float64), rng.integers(0, 3, size=(n, dim)).astype(np.float64)
        b[n // 2:] = b[:n - n // 2]
        return a, b
    return rng.uniform(0.0, 100.0, size=(m, dim)), rng.uniform(0.0, 100.0, size=(n, dim))


@pytest.mark.parametrize("dim", [1, 33, 64])
@pytest.mark.parametrize("integer", [False, True])
def test_match_numpy_equals_loop(dim, integer):
    a, b = descriptors(37, 53, dim, 11 + dim, integer)
    want, loop = mr.feature_match(a, b), mr.feature_match_loop(a, b)
    assert mr.same(want, loop, mr.MATCH_KEYS)
    if integer:
        ties = (want["fwd_d2"][:, 0] == want["fwd_d2"][:, 1]).sum()
        assert ties > 10 and (want["fwd_idx"][:, 0] < want["fwd_idx"][:, 1])[want["fwd_d2"][:, 0] == want["fwd_d2"][:, 1]].all()
    # symmetric bit for bit: the backward distances are the forward matrix's columns
    D = mr.dist_matrix(a, b)
    assert D.T.tobytes() == mr.dist_matrix(b, a).tobytes()


def test_match_padding():
    a, b = descriptors(5, 1, 33, 3)
    got = mr.feature_match(a, b)
    assert (got["fwd_idx"] == [[0, -1]] * 5).all() and np.isinf(got["fwd_d2"][:, 1]).all() and np.isfinite(got["fwd_d2"][:, 0]).all()
    assert got["bwd_idx"].shape == (1, 2) and (got["bwd_idx"] >= 0).all()
    assert mr.same(got, mr.feature_match_loop(a, b), mr.MATCH_KEYS)
    for m, n in ((0, 9), (9, 0)):
        got = mr.feature_match(np.zeros((m, 33)), np.zeros((n, 33)))
        assert got["fwd_idx"].shape == (m, 2) and got["bwd_idx"].shape == (n, 2) and (got["fwd_idx"] == -1).all() and (got["bwd_idx"] == -1).all()
        assert mr.same(got, mr.feature_match_loop(np.zeros((m, 33)), np.zeros((n, 33))), mr.MATCH_KEYS)


@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("ratio", [1.0, 0.8, 0.5])
def test_match_pairs_three_ways(mutual, ratio):
    a, b = descriptors(37, 53, 2, 5)   # (two dimensions: the ratio of the first to the second distance varies widely)
    mt = mr.feature_match(a, b)
    want = mr.match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, ratio)
    assert want.tobytes() == mr.match_pairs_loop(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, ratio).tobytes()
    got = mvicp.match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, ratio)
    assert got.dtype == np.int32 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert 0 < len(want) <= 37 and (np.diff(want[:, 0]) > 0).all()
    if not mutual and ratio == 1.0:
        assert len(want) == 37


def test_match_pairs_errors_and_padding(engine_lib):
    fi, fd = np.array([[0, -1], [-1, -1]], dtype=np.int32), np.array([[1.0, np.inf], [np.inf, np.inf]])
    bi = np.array([[0, 1]], dtype=np.int32)
    for ratio in (1.0, 0.5):   # the second place is padding: d0 <= r^2 inf holds
        assert mvicp.match_pairs(fi, fd, bi, True, ratio).tolist() == [[0, 0]] == mr.match_pairs(fi, fd, bi, True, ratio).tolist()
    assert mvicp.match_pairs(np.zeros((0, 2), np.int32), np.zeros((0, 2)), np.zeros((0, 2), np.int32)).shape == (0, 2)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    out = np.zeros((2, 2), np.int32)
    for ratio in (0.0, -1.0, float("nan")):
        assert engine_lib.mvicp_match_pairs(2, 1, vp(fi), vp(fd), vp(bi), 1, ratio, vp(out)) == ERR_ARG
    for args in ((None, vp(fd), vp(bi), 1, 1.0, vp(out)), (vp(fi), None, vp(bi), 1, 1.0, vp(out)), (vp(fi), vp(fd), None, 1, 1.0, vp(out)),
                 (vp(fi), vp(fd), vp(bi), 1, 1.0, None)):
        assert engine_lib.mvicp_match_pairs(2, 1, *args) == ERR_ARG
    assert engine_lib.mvicp_match_pairs(2, 0, vp(fi), vp(fd), vp(bi), 0, 1.0, vp(out)) == ERR_ARG   # j = 0 with n = 0
    with pytest.raises(ValueError):
        mr.match_pairs(fi, fd, bi, True, 0.0)


def test_sampler():
    for c, H, seed in ((3, 500, 0), (50, 300, 12345), (2 ** 31 - 1, 200, 2 ** 64 - 1)):
        idx = mr.sample_indices(seed, H, c)
        assert idx.shape == (H, 3) and idx.min() >= 0 and idx.max() < c
        assert all(int(idx[h, t]) == mr.sample_index(seed, h, t, c) for h in range(0, H, 7) for t in range(3))
    # splitmix64: the first outputs of the published generator from state 0 are the slots (h, t) = (0, 0), (0, 1), (0, 2), (1, 0)
    known = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC)
    for k, u in enumerate(known):
        assert mr.sample_index(0, k // 3, k % 3, 2 ** 31 - 1) == ((u >> 32) * (2 ** 31 - 1)) >> 32
    assert [mr.sample_index(12345, 0, t, 432) for t in range(3)] == [int(v) for v in mr.sample_indices(12345, 1, 432)[0]]
    # all c values are drawn, about evenly
    hist = np.bincount(mr.sample_indices(7, 30000, 50).ravel(), minlength=50)
    assert hist.min() > 1500 and hist.max() < 2100


def lattice_case():
    rng = np.random.Generator(np.random.PCG64(21))
    P = rng.integers(-4, 5, size=(50, 3)).astype(np.float64)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Q = P @ Rz.T + np.array([2.0, -3.0, 5.0])
    Q[::5] += rng.integers(-2, 3, size=(10, 3))     # a fifth of the pairs are wrong
    return np.ascontiguousarray(P), np.ascontiguousarray(Q)


@pytest.mark.parametrize("edge_sim", [0.0, 0.9])
def test_consensus_numpy_equals_loop(edge_sim):
    P, Q = lattice_case()
    for seed in (1, 99):
        want = mr.consensus(P, Q, 300, seed, 1.0, edge_sim)
        assert mr.same(want, mr.consensus_loop(P, Q, 300, seed, 1.0, edge_sim), mr.CONSENSUS_KEYS)
        assert 0 < want["accepted"] < 300 and want["best"] >= 0 and want["count"] == want["flags"].sum() == want["counts"].max()
        assert (want["counts"] >= 0).sum() == want["accepted"] and want["best"] == int(np.flatnonzero(want["counts"] == want["count"])[0])
    rng = np.random.Generator(np.random.PCG64(4))
    P, Q = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    want = mr.consensus(P, Q, 300, 5, 0.3, edge_sim)
    assert mr.same(want, mr.consensus_loop(P, Q, 300, 5, 0.3, edge_sim), mr.CONSENSUS_KEYS)


def test_consensus_all_rejected():
    P = np.outer(np.arange(20.0), [1.0, 2.0, -1.0])   # collinear: no triangle has a frame
    want = mr.consensus(P, P.copy(), 200, 3, 1.0, 0.0)
    assert want["best"] == -1 and want["count"] == 0 and want["accepted"] == 0 and (want["counts"] == -1).all() and not want["flags"].any()
    assert want["pose"].tobytes() == np.eye(4).tobytes()
    assert mr.same(want, mr.consensus_loop(P, P.copy(), 200, 3, 1.0, 0.0), mr.CONSENSUS_KEYS)


def test_accepted_poses_are_rigid():
    cl, ref = mr.e2e_clouds(False), mr.e2e_reference(False)
    P, Q = ref["P"], ref["Q"]
    ok, R, t, idx = mr.hypotheses(P, Q, 2000, mr.E2E_SEED, mr.E2E_EDGE_SIM)
    assert 50 < ok.sum() < 1000
    R, t, idx = R[ok], t[ok], idx[ok]
    assert np.abs(R @ np.transpose(R, (0, 2, 1)) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
    cp, cq = P[idx].mean(1), Q[idx].mean(1)
    assert np.abs(np.einsum("hrk,hk->hr", R, cp) + t - cq).max() < 1e-12
    assert cl["truth"].shape == (4, 4)


@pytest.mark.parametrize("partial", [False, True])
def test_end_to_end_pose(partial):
    """Measured with matchref on the CPU: full overlap 0.533 deg, 0.533 spacings (432 mutual pairs, 689 accepted hypotheses, a winner
    with 131 inliers); partial overlap 1.199 deg, 1.021 spacings (350 pairs, 314 accepted, 79 inliers).  The bound of 3 deg and 3
    spacings leaves a factor >= 2.5."""
    cl, ref = mr.e2e_clouds(partial), mr.e2e_reference(partial)
    cons = ref["consensus"]
    deg, dt = mr.pose_error(cons["pose"], cl["truth"])
    print("partial" if partial else "full", "pairs", len(ref["pairs"]), "accepted", cons["accepted"], "inliers", cons["count"], "deg", deg,
          "spacings", dt / cl["spacing"])
    assert len(ref["pairs"]) >= 100 and len(ref["pairs"]) % 64 != 0 and cons["best"] >= 0
    assert deg < 3.0 and dt < 3.0 * cl["spacing"]
    assert cons["accepted"] < 0.1 * mr.E2E_H     # edge_sim = 0.9 rejects more than 90 % on real matches


def test_bumps_is_one_surface():
    p1, n1 = mr.bumps(500, 100)
    p2, _ = mr.bumps(500, 100)
    assert p1.tobytes() == p2.tobytes() and np.abs(np.linalg.norm(n1, axis=1) - 1).max() < 1e-15 and (n1[:, 2] > 0).all()
    # the analytic normals are the field's: a central difference of the height agrees
    q, _ = mr.bumps(500, 200, 0.3, 1.3)
    assert q[:, 0].min() >= 0.3 and q[:, 0].max() <= 1.3 and np.ptp(p1[:, 2]) > 0.05
    c, a, s = mr._bump_field()
    z = lambda x, y: (a * np.exp(-((x - c[:, 0]) ** 2 + (y - c[:, 1]) ** 2) / (2 * s ** 2))).sum()
    h = 1e-6
    for i in range(0, 500, 50):
        x, y = p1[i, 0], p1[i, 1]
        g = np.array([-(z(x + h, y) - z(x - h, y)) / (2 * h), -(z(x, y + h) - z(x, y - h)) / (2 * h), 1.0])
        assert np.abs(g / np.linalg.norm(g) - n1[i]).max() < 1e-8 and abs(z(x, y) - p1[i, 2]) < 1e-15


def test_header_and_binding_agree(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    for name in ("mvicp_feature_match", "mvicp_feature_match_fetch", "mvicp_match_pairs", "mvicp_consensus", "mvicp_consensus_fetch"):
        assert re.search(r"\b%s\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)
    assert C.sizeof(L.ConsensusResult) == 16 + 128
    assert callable(mvicp.match_pairs) and callable(mvicp.coarse_align) and hasattr(mvicp.Engine, "feature_match") and hasattr(mvicp.Engine, "consensus")
