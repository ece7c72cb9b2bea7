"""The cases of tests/pathcases.py reach the branch each is built for, and none is trivial: asserted on the launch plan (the host arithmetic
restated from the sources' own constants) and on the numpy references alone, without a GPU.  tests/test_gpu_paths.py,
test_gpu_outlier.py and test_gpu_voxel.py run the same cases on the device.  A constant that changes so that a case no longer reaches
its branch fails here."""
import os
import shutil

import numpy as np
import pytest

import matchref as mr
import pathcases as pc
import voxelref


# ---- the constants and the plans
def test_constants_are_read_from_the_sources_by_name(tmp_path):
    k = pc.CONSTANTS
    assert set(k["consensus"]) == {"kThreads", "kPairTile", "kWantBlocks"}
    assert set(k["match"]) == {"kThreads", "kTile", "kGenRows", "kGenTile", "kMaxChunks"}
    assert len(k["outlier"]) == 3 and all(cap == kmax + 1 for kmax, cap in k["outlier"])     # a list holds the point itself and k neighbours
    # a name that is not there raises, whichever file misses it
    for name, old, new in (("consensus.hip", "kWantBlocks", "kBlocksWanted"), ("match.hip", "constexpr int kGenTile", "constexpr long kGenTile"),
                           ("outlier.hip", "else if (k <= ", "else if (k < ")):
        d = tmp_path / name.replace(".", "_")
        d.mkdir()
        for f in ("consensus.hip", "match.hip", "outlier.hip"):
            shutil.copy(os.path.join(pc.CSRC, f), d / f)
        text = (d / name).read_text()
        assert old in text
        (d / name).write_text(text.replace(old, new))
        with pytest.raises(LookupError):
            pc.load_constants(str(d))


def test_plans_restate_the_host_arithmetic():
    kc, km = pc.CONSTANTS["consensus"], pc.CONSTANTS["match"]
    # consensus(): the shapes of tests/test_gpu_match.py never walk two tiles in one workgroup
    for c, acc in ((1101, 7200), (125, 1900), (20, 100), (3, 40)):
        p = pc.consensus_plan(c, acc)
        assert p["tiles_per_block"] == 1 and p["gy"] == p["tiles"], (c, acc, p)
    p = pc.consensus_plan(10 * kc["kPairTile"] * kc["kWantBlocks"] + 1, 1)
    assert p["gx"] == 1 and p["tiles_per_block"] == 11 and p["rows_in_last_block"] == kc["kWantBlocks"] * kc["kPairTile"] * 10 + 1 - (p["gy"] - 1) * p["per_y"]
    assert (p["gy"] - 1) * p["per_y"] < 10 * kc["kPairTile"] * kc["kWantBlocks"] + 1 <= p["gy"] * p["per_y"]
    # every pair is covered exactly once, whatever the sizes
    rng = np.random.Generator(np.random.PCG64(1))
    for c, acc in zip(rng.integers(3, 400000, size=200).tolist(), rng.integers(1, 200000, size=200).tolist()):
        p = pc.consensus_plan(c, acc)
        assert p["gy"] >= 1 and (p["gy"] - 1) * p["per_y"] < c <= p["gy"] * p["per_y"] and 1 <= p["rows_in_last_block"] <= p["per_y"]
        assert p["per_y"] % kc["kPairTile"] == 0 or p["per_y"] == c
        assert pc.consensus_gx_from_bytes(pc.consensus_score_bytes(p, c, acc), c, acc) == p["gx"]
    # chunking(): the chunk sizes of tests/test_gpu_match.py are whole tiles or smaller than one
    for chunk in (1, 64, 2048):
        for right in (257, 130, 70, 9):
            for dim in (33, 64):
                p = pc.match_plan(chunk, 10, right, dim)
                assert not p["clamped"] and (p["chunk"] % p["tile"] == 0 or p["chunk"] < p["tile"] or p["chunks"] == 1), (chunk, right, p)
    for ch, right in zip(rng.integers(1, 5000, size=200).tolist(), rng.integers(1, 300000, size=200).tolist()):
        for dim in (33, 5):
            p = pc.match_plan(ch, 77, right, dim)
            assert 1 <= p["chunks"] <= km["kMaxChunks"] and (p["chunks"] - 1) * p["chunk"] < right <= p["chunks"] * p["chunk"]
            assert pc.match_chunks_from_bytes(pc.match_bytes(p, 77, right, dim), p["wgs"], 77, right, dim) == p["chunks"]


# ---- consensus
@pytest.mark.parametrize("name", ["C1", "C2", "C3", "C4"])
def test_consensus_cases_reach_their_paths(name):
    plan, want = pc.check_consensus_case(name)
    P, Q, H = pc.consensus_pairs(name)
    assert (len(P), H) == pc.CONS_SHAPES[name] and len(want["counts"]) == H
    print(name, "plan", plan, "accepted", want["accepted"], "count", want["count"], "distinct", len(np.unique(want["counts"])))


def test_consensus_reference_equals_the_scalar_loop_on_a_slice_of_c3():
    """the vectorised reference against the scalar statement, on this module's own data (a shortened C3: the loop is slow)"""
    P, Q, _ = pc.consensus_pairs("C3")
    a = mr.consensus(P[:300], Q[:300], 40, pc.CONS_SEED, pc.CONS_TAU, pc.CONS_EDGE_SIM)
    b = mr.consensus_loop(P[:300], Q[:300], 40, pc.CONS_SEED, pc.CONS_TAU, pc.CONS_EDGE_SIM)
    assert mr.same(a, b, mr.CONSENSUS_KEYS) and a["accepted"] > 30


@pytest.mark.parametrize("change", [("kWantBlocks", 256), ("kWantBlocks", 4096), ("kPairTile", 128), ("kPairTile", 512), ("kThreads", 128)])
def test_a_changed_consensus_constant_is_noticed(change):
    """every case is tied to the constants: with another value at least one case no longer reaches its branch, and says so"""
    k = dict(pc.CONSTANTS["consensus"])
    k[change[0]] = change[1]
    failed = []
    for name in ("C1", "C2", "C3"):
        try:
            pc.check_consensus_case(name, k)
        except AssertionError:
            failed.append(name)
    assert failed, change


# ---- matching
@pytest.mark.parametrize("dim", pc.MATCH_DIMS)
def test_m1_the_chunk_count_clamp(dim):
    fwd, bwd, want = pc.check_match_case("M1", dim, 1)
    assert want["fwd_idx"].shape == (3, 2) and want["bwd_idx"].shape == (70000, 2) and len(np.unique(want["bwd_idx"][:, 0])) == 3
    print("M1", dim, "fwd", fwd, "bwd", bwd)


@pytest.mark.parametrize("dim", pc.MATCH_DIMS)
def test_m2_chunks_that_end_inside_a_tile(dim):
    fwd, bwd, want = pc.check_match_case("M2", dim, pc.M2_CHUNK)
    print("M2", dim, "fwd", fwd, "bwd", bwd)


@pytest.mark.parametrize("order", ["a", "b", "c"])
def test_m3_the_early_exit(order):
    pc.check_match_case("M3" + order, 33)
    a, b = pc.match_m3(order)
    assert mr.same(mr.feature_match(a[60:70], b[:80]), mr.feature_match_loop(a[60:70], b[:80]), mr.MATCH_KEYS)


@pytest.mark.parametrize("dim", pc.MATCH_DIMS)
def test_m4_squares_that_overflow(dim):
    for chunk in (pc.MATCH_DEFAULT_CHUNK, 64):
        fwd, bwd, want = pc.check_match_case("M4", dim, chunk)
    assert bwd["chunks"] > 1 and fwd["chunks"] > 1          # with chunks of 64 the all-infinite lists go through the merge
    a, b = pc.match_m4(dim)
    with np.errstate(over="ignore"):
        assert mr.same(mr.feature_match(a[:8], b[:30]), mr.feature_match_loop(a[:8], b[:30]), mr.MATCH_KEYS)


@pytest.mark.parametrize("change", [("kMaxChunks", 70000), ("kMaxChunks", 1024), ("kTile", 50), ("kTile", 100), ("kGenTile", 50), ("kGenTile", 20),
                                    ("kThreads", 512)])
def test_a_changed_match_constant_is_noticed(change):
    k = dict(pc.CONSTANTS["match"])
    k[change[0]] = change[1]
    failed = []
    for name, chunk in (("M1", 1), ("M2", pc.M2_CHUNK)):
        for dim in pc.MATCH_DIMS:
            try:
                pc.check_match_case(name, dim, chunk, k)
            except AssertionError:
                failed.append((name, dim))
    assert failed, change


# ---- the outlier filter
def test_outlier_sweep_straddles_every_capacity_boundary():
    assert pc.OUTLIER_SWEEP_K == pc.outlier_boundary_ks()
    caps = [pc.outlier_capacity(k) for k in pc.OUTLIER_SWEEP_K]
    assert caps[0] == caps[1] < caps[2] == caps[3] < caps[4] == caps[5] and sorted(set(caps)) == [c for _, c in pc.CONSTANTS["outlier"]]
    for table in ([(7, 9), (16, 17), (32, 33)], [(8, 9), (15, 17), (32, 33)], [(8, 9), (24, 25), (32, 33)]):    # a threshold that moves is noticed
        assert pc.OUTLIER_SWEEP_K != pc.outlier_boundary_ks(table)


@pytest.mark.parametrize("params", pc.O1_PARAMS)
def test_o1_far_from_the_origin(params):
    want = pc.check_outlier_far(*params)
    assert {pc.outlier_capacity(k) for k, _, _ in pc.O1_PARAMS} == {c for _, c in pc.CONSTANTS["outlier"]}     # one case per capacity
    print("O1", params, "kept", want["stats"]["kept"])


# ---- the voxel grid
@pytest.mark.parametrize("shift", [pc.V1_SHIFT, pc.V1_SHIFT_WIDER])
@pytest.mark.parametrize("h", pc.V1_VOXELS)
def test_v1_wide_keys(shift, h):
    bits, want = pc.check_voxel_v1(shift, h)
    assert bits == (60 if shift == pc.V1_SHIFT else 61)
    p, _ = pc.voxel_two_clusters(shift)
    assert voxelref.cells(p, h).min() < -400000 and voxelref.cells(p, h).max() > 400000      # negative cells of large magnitude
    print("V1", shift, h, "bits", bits, "voxels", len(want["cnt"]), "multi", int((want["cnt"] > 1).sum()))


def test_v1_refused_extent():
    p, nr = pc.voxel_two_clusters(pc.V1_SHIFT_REFUSED)
    for h in pc.V1_VOXELS:
        assert pc.voxel_key_bits(p, h)[1] >= 2 ** 62
        with pytest.raises(ValueError, match="too small for the extent"):
            voxelref.voxel_grid([p], [nr], h)
    assert len(voxelref.voxel_grid([p], [nr], 0.04)["cnt"]) == 2


def test_v2_georeferenced_and_fused():
    want = pc.check_voxel_v2()
    print("V2", "voxels", len(want["cnt"]), "multi", int((want["cnt"] > 1).sum()))
