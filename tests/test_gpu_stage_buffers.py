"""The buffers behind eleven library-owned results (voxel grid, outlier filter, neighbour search, FPFH, ISS keypoints, descriptor
matching, consensus, batched coarse poses, clusters, the dominant plane, boundary points -- the last three with their selections) on the
MI355X: each stage grows its buffers on demand, keeps the larger ones for a smaller call and derives its result views anew inside them,
and mvicp_set_num_frames releases all of it.  Every fetched result equals the
stage's numpy reference byte for byte; no tolerance anywhere.  Sizes: about 64, then about 700, then about 64 points (rows, pairs) on
ONE engine without a release in between, so the second call grows every buffer and the third runs inside the larger ones."""
import ctypes as C
import functools

import numpy as np
import pytest

import boundref
import clusterref
import fpfhref
import initref
import issref
import knnref
import matchref
import mvicp
import normref
import outlierref
import planeref
import voxelref
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_STATE = -3
SIZES = (64, 700, 61)            # small, large, small again (another cloud, so that a stale view or size cannot pass)
RADIUS = {64: 0.3, 700: 0.1, 61: 0.3}   # the sheet holds n points per square metre: about 18 / 22 / 17 points within the radius
VOXEL = {64: 0.2, 700: 0.05, 61: 0.2}
H, TAU, EDGE_SIM, DIM = 200, 0.03, 0.9, 33
STAGES = ("voxel", "outlier", "knn", "knn_all", "fpfh", "iss", "match", "consensus", "coarse", "cluster", "plane", "boundary")
# the row-selecting stages: cluster(RADIUS / 2, min_pts 4) + select(min_size 5); segment_plane(tau, H, seed 7 + n, refit) and boundary(max_nn,
# cos_gap, source 0) + both selections.  What the references give, so that no case can pass by selecting nothing or everything
CLUSTER_MIN_PTS, CLUSTER_MIN_SIZE, PLANE_TAU, BOUNDARY_NN, BOUNDARY_COS = 4, 5, 0.01, 12, -0.5
CLUSTERS_NOISE = {64: (4, 9), 700: (9, 37), 61: (3, 7)}
PLANE_INLIERS = {64: 62, 700: 686, 61: 59}
BOUNDARY_FLAGGED = {64: 41, 700: 362, 61: 40}


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def cloud(n):
    p, nr, _ = outlierref.sheet_cloud(n, 100 + n)
    return p, nr


@functools.lru_cache(maxsize=None)
def queries(n):
    return np.random.Generator(np.random.PCG64(200 + n)).uniform(-0.5, 0.7, size=(n + 3, 3))


@functools.lru_cache(maxsize=None)
def tables(n):
    """-> (A (n, 33), B (n - 4, 33)): integer-valued descriptors, so first and second places tie exactly"""
    rng = np.random.Generator(np.random.PCG64(300 + n))
    return rng.integers(0, 3, size=(n, DIM)).astype(np.float64), rng.integers(0, 3, size=(n - 4, DIM)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def pairs(n):
    """-> (P, Q): n index-aligned pairs, Q = P moved by a pose with 1 cm of noise and a fifth of the rows replaced"""
    rng = np.random.Generator(np.random.PCG64(400 + n))
    P = rng.uniform(0.0, 1.0, size=(n, 3))
    Q = P @ synth.so3_exp(rng.uniform(-1.0, 1.0, size=3)).T + rng.uniform(-0.5, 0.5, size=3) + rng.normal(0.0, 0.01, size=(n, 3))
    bad = rng.random(n) < 0.2
    Q[bad] = rng.uniform(0.0, 1.0, size=(int(bad.sum()), 3))
    return np.ascontiguousarray(P), np.ascontiguousarray(Q)


@functools.lru_cache(maxsize=None)
def coarse_sets(n):
    """-> (desc, xyz, offsets) of two sets of n and n - 4 rows that mostly match i <-> i"""
    rng = np.random.Generator(np.random.PCG64(500 + n))
    base_d = rng.integers(0, 3, size=(n, DIM)).astype(np.float64)
    P, Q = pairs(n)
    desc = np.concatenate([base_d, base_d[:n - 4]])
    xyz = np.concatenate([P, Q[:n - 4]])
    return np.ascontiguousarray(desc), np.ascontiguousarray(xyz), np.array([0, n, 2 * n - 4], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def reference(stage, n):
    p, nr = cloud(n)
    if stage == "voxel":
        return voxelref.voxel_grid([p], [nr], VOXEL[n])
    if stage == "outlier":
        return outlierref.outlier_filter(p, nr, 8, 1.0, RADIUS[n])
    if stage == "knn":
        return knnref.knn_search(p, queries(n), 8, 0.0)
    if stage == "knn_all":
        return knnref.knn_search(p, queries(n), 0, RADIUS[n])
    if stage == "fpfh":
        return fpfhref.fpfh(p, nr, RADIUS[n], 16)
    if stage == "iss":
        return issref.iss(p, RADIUS[n], RADIUS[n], 0.975, 0.975, 3)
    if stage == "match":
        return matchref.feature_match(*tables(n))
    if stage == "consensus":
        return matchref.consensus(*pairs(n), H, 7 + n, TAU, EDGE_SIM)
    if stage == "cluster":
        return clusterref.cluster(p, nr, RADIUS[n] / 2, CLUSTER_MIN_PTS)
    if stage == "plane":
        return planeref.segment(p, nr, PLANE_TAU, H, 7 + n)
    if stage == "boundary":
        return boundref.boundary(p, nr, BOUNDARY_NN, 0.0, BOUNDARY_COS)
    desc, xyz, off = coarse_sets(n)
    return [initref.coarse_edge(desc[a0:a1], xyz[a0:a1], desc[b0:b1], xyz[b0:b1], True, 1.0, H, seed, TAU, EDGE_SIM)
            for (a0, a1, b0, b1), seed in ((((off[0], off[1], off[1], off[2])), 11 + n), ((off[1], off[2], off[0], off[1]), 12 + n))]


def check(eng, stage, n, frame, device=False):
    """one call of `stage` on the input of size n (its cloud is frame `frame` of the engine) and the fetch, against the reference"""
    what = (stage, n, "device" if device else "host")
    want = reference(stage, n)
    host = lambda r: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    if stage == "voxel":
        assert 1 < len(want["cnt"]) < n, what
        assert voxelref.same(host(eng.voxel_grid(VOXEL[n], frames=[frame], device=device)), want), what
    elif stage == "outlier":
        assert 0 < len(want["idx"]) < n, what
        assert outlierref.same(host(eng.outlier_filter(frame, 8, 1.0, RADIUS[n], device=device)), want), what
    elif stage == "knn":
        assert knnref.same(host(eng.knn_search(frame, queries(n), 8, 0.0, device=device)), want), what
    elif stage == "knn_all":
        assert int(want["total"]) > n, what
        assert knnref.same(host(eng.knn_search(frame, queries(n), 0, RADIUS[n], device=device)), want), what
    elif stage == "fpfh":
        assert 2 < int(want["used"].max()) and int(want["used"].min()) < 16, what
        assert fpfhref.same(host(eng.fpfh(frame, RADIUS[n], 16, device=device)), want, ("desc", "used")), what
    elif stage == "iss":
        assert len(want["idx"]) > 0, what
        assert issref.same(host(eng.iss_keypoints(frame, RADIUS[n], RADIUS[n], 0.975, 0.975, 3, device=device)), want), what
    elif stage == "match":
        assert matchref.same(host(eng.feature_match(*tables(n), device=device)), want, matchref.MATCH_KEYS), what
    elif stage == "consensus":
        assert want["accepted"] > 0 and want["count"] > n // 2, what
        assert matchref.same(eng.consensus(*pairs(n), H, 7 + n, TAU, EDGE_SIM), want, matchref.CONSENSUS_KEYS), what
    elif stage == "cluster":
        p, nr = cloud(n)
        assert (want["stats"]["clusters"], want["stats"]["noise"]) == CLUSTERS_NOISE[n], what
        assert clusterref.same(host(eng.cluster(frame, RADIUS[n] / 2, CLUSTER_MIN_PTS, device=device)), want), what
        ws = clusterref.select(p, nr, want, CLUSTER_MIN_SIZE, 0)
        assert 0 < ws["kept"] < n, what
        assert clusterref.same_kept(host(eng.cluster_select(CLUSTER_MIN_SIZE, 0, device=device)), ws), what
    elif stage == "plane":
        p, nr = cloud(n)
        assert int(want["flags"].sum()) == want["count_refined"] == PLANE_INLIERS[n] and want["refit"] == 1, what
        assert planeref.same(host(eng.segment_plane(frame, PLANE_TAU, H, 7 + n, device=device)), want), what
        for inliers in (True, False):
            assert planeref.same_kept(host(eng.plane_select(inliers, device=device)), planeref.select(p, nr, want, inliers)), (what, inliers)
    elif stage == "boundary":
        p, nr = cloud(n)
        assert want["boundary"] == BOUNDARY_FLAGGED[n], what
        assert boundref.same(host(eng.boundary(frame, BOUNDARY_NN, 0.0, BOUNDARY_COS, device=device)), want), what
        for flagged in (True, False):
            assert boundref.same_kept(host(eng.boundary_select(flagged, device=device)), boundref.select(p, nr, want, flagged)), (what, flagged)
    else:
        desc, xyz, off = coarse_sets(n)
        res = eng.coarse_pairs(desc, xyz, off, [0, 1], [1, 0], [11 + n, 12 + n], True, 1.0, H, TAU, EDGE_SIM)
        for e, w in enumerate(want):
            assert w["pairs_n"] > n // 2 and w["count"] > 0, (what, e)
            for key, ref_key in (("pairs", "pairs_n"), ("best", "best"), ("count", "count"), ("accepted", "accepted")):
                assert int(res[key][e]) == int(w[ref_key]), (what, e, key)
            assert res["pose"][e].tobytes() == np.ascontiguousarray(w["pose"]).tobytes(), (what, e, "pose")
            got_pairs, got_flags = eng.coarse_pairs_fetch(e, device=device)
            if device:
                got_pairs, got_flags = got_pairs.cpu().numpy(), got_flags.cpu().numpy()
            assert got_pairs.dtype == np.int32 and got_pairs.shape == w["pairs"].shape and got_pairs.tobytes() == w["pairs"].tobytes(), (what, e, "pairs")
            assert got_flags.dtype == np.uint8 and got_flags.shape == w["flags"].shape and got_flags.tobytes() == w["flags"].tobytes(), (what, e, "flags")


def upload(eng):
    eng.set_frames([cloud(n)[0] for n in SIZES], [cloud(n)[1] for n in SIZES])


@pytest.mark.parametrize("stage", STAGES)
def test_small_large_small(eng, stage):
    """grow, keep the larger buffer, views derived anew inside the larger arena: a fresh set of buffers, then three calls"""
    upload(eng)   # (mvicp_set_num_frames: the stage starts without buffers)
    for frame, n in enumerate(SIZES):
        check(eng, stage, n, frame, device=(frame == 2))


def fetch_statuses(eng):
    """every fetch entry point on the context as it is -> [(status, message)]"""
    lib, h = eng.lib, eng.h
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data_as(C.c_void_p)
    calls = (lambda: lib.mvicp_voxel_fetch(h, 1, p, None, None),
             lambda: lib.mvicp_outlier_fetch(h, 1, p, None, None, 1, None, None),
             lambda: lib.mvicp_knn_fetch(h, 1, 1, p, None, None, None),
             lambda: lib.mvicp_fpfh_fetch(h, 1, p, None),
             lambda: lib.mvicp_iss_fetch(h, 1, p, None, None, 1, None, None, None),
             lambda: lib.mvicp_feature_match_fetch(h, 1, 1, p, None, None, None),
             lambda: lib.mvicp_consensus_fetch(h, 1, p, 1, None),
             lambda: lib.mvicp_coarse_pairs_fetch(h, 0, 1, p, None),
             lambda: lib.mvicp_cluster_fetch(h, 1, p, None, 1, None),
             lambda: lib.mvicp_cluster_fetch_kept(h, 1, p, None, None, None),
             lambda: lib.mvicp_plane_fetch(h, 1, p, 1, None),
             lambda: lib.mvicp_plane_fetch_kept(h, 1, p, None, None),
             lambda: lib.mvicp_boundary_fetch(h, 1, p, None, None, None),
             lambda: lib.mvicp_boundary_fetch_kept(h, 1, p, None, None))
    out = []
    for call in calls:
        st = call()
        out.append((st, lib.mvicp_last_error()))
    return out


FIRST = (b"call mvicp_voxel_grid first", b"call mvicp_outlier_filter first", b"call mvicp_knn_search first", b"call mvicp_fpfh first",
         b"call mvicp_iss_keypoints first", b"call mvicp_feature_match first", b"call mvicp_consensus first", b"call mvicp_coarse_pairs first",
         b"call mvicp_cluster first", b"call mvicp_cluster first", b"call mvicp_segment_plane first", b"call mvicp_segment_plane first",
         b"call mvicp_boundary first", b"call mvicp_boundary first")


def test_set_num_frames_releases_every_result(eng):
    upload(eng)
    for stage in STAGES:
        check(eng, stage, SIZES[1], 1)
    for (st, msg), first in zip(fetch_statuses(eng), FIRST):
        assert st != ERR_STATE, (st, msg)   # (a result is there: whatever the tiny capacities give, it is not "call ... first")
    upload(eng)   # mvicp_set_num_frames and the frames again
    for (st, msg), first in zip(fetch_statuses(eng), FIRST):
        assert st == ERR_STATE and first in msg, (st, msg, first)
    for stage in STAGES:
        check(eng, stage, SIZES[0], 0)
    for (st, msg), first in zip(fetch_statuses(eng), FIRST):
        assert st != ERR_STATE, (st, msg)


def _stages_on_a_frame_without_normals(eng, n):
    """the 61-point sheet uploaded WITHOUT normals; cluster, segment_plane, estimate_normals + boundary(source 1) -> (the estimate = what
    adopt_normals will store, the three references; the boundary's is by the estimate)"""
    p, _ = cloud(n)
    N = normref.normals(p, BOUNDARY_NN)
    bnd = boundref.boundary(p, N["nrm"], BOUNDARY_NN, 0.0, BOUNDARY_COS)
    assert 0 < bnd["boundary"] < n
    eng.set_frames([p], None)
    assert eng.cluster(0, RADIUS[n] / 2, CLUSTER_MIN_PTS)["stats"]["has_normals"] == 0
    assert eng.segment_plane(0, PLANE_TAU, H, 7 + n)["has_normals"] == 0
    assert normref.same(eng.estimate_normals(0, BOUNDARY_NN), N)
    assert boundref.same(eng.boundary(0, BOUNDARY_NN, 0.0, BOUNDARY_COS, source=1), bnd)
    return np.ascontiguousarray(N["nrm"]), reference("cluster", n), reference("plane", n), bnd


def _selections(eng, n, N, clu, pla, bnd, device):
    """every selection of the three results against its reference given the frame's normals N (None: it stores none)"""
    p, _ = cloud(n)
    host = lambda r: {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    what = (device, N is not None)
    assert clusterref.same_kept(host(eng.cluster_select(CLUSTER_MIN_SIZE, 0, device=device)), clusterref.select(p, N, clu, CLUSTER_MIN_SIZE, 0)), what
    for wanted in (True, False):
        assert planeref.same_kept(host(eng.plane_select(wanted, device=device)), planeref.select(p, N, pla, wanted)), (what, wanted)
        assert boundref.same_kept(host(eng.boundary_select(wanted, device=device)), boundref.select(p, N, bnd, wanted)), (what, wanted)


def test_normals_that_arrive_between_the_stage_and_the_selection(eng):
    """A selection carries normals iff its frame has stored normals when the SELECTION runs: adopt_normals between the stage and the
    selection puts them into the rows, with host and with device destinations."""
    n = SIZES[2]
    N, clu, pla, bnd = _stages_on_a_frame_without_normals(eng, n)
    eng.adopt_normals()
    for device in (False, True):
        _selections(eng, n, N, clu, pla, bnd, device)
    for sel in (clusterref.select(cloud(n)[0], N, clu, CLUSTER_MIN_SIZE, 0), planeref.select(cloud(n)[0], N, pla, False), boundref.select(cloud(n)[0], N, bnd, False)):
        assert sel["kept"] > 0 and sel["nrm"].shape == (sel["kept"], 3) and np.abs(sel["nrm"]).max() > 0.5   # (normals are present, and not zeros)


def test_a_selection_made_before_the_normals_arrived_carries_none(eng):
    """The reverse order: select, then adopt_normals, then fetch again -- the rows are those of the selection, without normals, and asking
    for nrm is MVICP_ERR_STATE."""
    n = SIZES[2]
    N, clu, pla, bnd = _stages_on_a_frame_without_normals(eng, n)
    for device in (False, True):
        _selections(eng, n, None, clu, pla, bnd, device)
    eng.adopt_normals()
    lib, h, p = eng.lib, eng.h, cloud(n)[0]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for fetch, want in ((lambda *a: lib.mvicp_cluster_fetch_kept(h, n, *a, None), clusterref.select(p, None, clu, CLUSTER_MIN_SIZE, 0)),
                        (lambda *a: lib.mvicp_plane_fetch_kept(h, n, *a), planeref.select(p, None, pla, False)),
                        (lambda *a: lib.mvicp_boundary_fetch_kept(h, n, *a), boundref.select(p, None, bnd, False))):
        xyz, nrm, idx = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
        assert fetch(None, vp(nrm), None) == ERR_STATE and b"normals" in lib.mvicp_last_error() and not nrm.any()
        assert fetch(vp(xyz), None, vp(idx)) == 0
        k = want["kept"]
        assert 0 < k < n and xyz[:k].tobytes() == np.ascontiguousarray(want["xyz"]).tobytes() and idx[:k].tobytes() == want["idx"].tobytes()
    # the next selection of the same results sees the normals
    _selections(eng, n, N, clu, pla, bnd, False)
