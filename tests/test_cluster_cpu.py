"""The contract of mvicp_cluster on the CPU: tests/clusterref.py's numpy form equals its scalar loop, scipy's connected components and
sklearn's DBSCAN where those define the same thing; mvicp_cluster_keep_rule through the C ABI equals the reference rule; the argument
errors need no GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import clusterref as cr
import mvicp
import outlierref
import traverseref
from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("mvicp_cluster", "mvicp_cluster_fetch", "mvicp_cluster_keep_rule", "mvicp_cluster_select", "mvicp_cluster_fetch_kept")


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> (points, radius, the min_pts to run); the helix subsampled to 600 points for the loop (its radius scaled with the spacing)."""
    blobs = cr.blobs_cloud()[0][:700]
    helix = cr.helix_cloud(4096)[::7][:600]
    step = float(np.linalg.norm(helix[1] - helix[0]))
    R = float(np.nextafter(cr.LATTICE_PITCH, 1.0))
    return {
        "blobs": (blobs, 0.035, (1, 5, 17)),
        "sheet+clump": (cr.sheet_clump_cloud()[0][2700:], 0.12, (1, 4)),
        "lattice, radius = pitch": (cr.dyadic_lattice(), cr.LATTICE_PITCH, (1, 2)),
        "lattice": (cr.dyadic_lattice(), R, (1, 5, 6, 7)),
        "bridge": (cr.bridge_cloud()[0], cr.BRIDGE_RADIUS, (1, cr.BRIDGE_MIN_PTS)),
        "helix": (helix, 1.5 * step, (2, 3)),
        "identical": (np.tile([[0.25, -0.5, 1.0]], (40, 1)), 0.01, (1, 40, 41)),
        "line": (cr.line_cloud()[:200], 0.03, (1, 3, 5)),
        "far patch": (traverseref.patch_cloud("far"), 0.0301, (1, 5, 9)),
        "corner patch": (traverseref.patch_cloud("corner"), 0.0401, (1, 3)),
        "lattice + far cluster": (outlierref.lattice_cloud()[0], 0.0076, (1, 8)),
        "two": (np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]]), 0.0101, (1, 2, 3)),
    }


@pytest.mark.parametrize("name", sorted(clouds()))
def test_numpy_form_equals_the_scalar_loop(name):
    p, radius, mins = clouds()[name]
    seen = set()
    for m in mins:
        got, want = cr.cluster(p, None, radius, m), cr.cluster_loop(p, None, radius, m)
        assert cr.same(got, want), (name, m, got["stats"], want["stats"])
        s = got["stats"]
        assert s["core"] + s["border"] + s["noise"] == len(p) and int(got["size"].sum()) == s["core"] + s["border"]
        assert (got["label"][got["core"] == 1] >= 0).all()
        seen.add((s["clusters"], s["core"], s["border"], s["noise"]))
        for rule in ((0, 0), (3, 0), (0, 1), (2, 2)):
            sel = cr.select(p, None, got, *rule)
            assert (np.diff(sel["idx"]) > 0).all() and (sel["label"] >= 0).all() and sel["xyz"].tobytes() == p[sel["idx"]].tobytes()
    assert len(seen) > 1 or len(mins) == 1, (name, seen)   # min_pts changes the answer: the clouds are not trivial


def test_the_bridge_and_the_lattice_hold_what_they_are_for():
    p, mid = cr.bridge_cloud()
    r = cr.cluster(p, None, cr.BRIDGE_RADIUS, cr.BRIDGE_MIN_PTS)
    assert r["stats"]["clusters"] == 2 and r["stats"]["noise"] == 0 and not r["core"][mid]
    D = cr.dist2_slab(p, 0)[mid]
    near = np.flatnonzero(cr.adjacency(p, cr.BRIDGE_RADIUS)[mid] & (r["core"] == 1))
    first = near[D[near] == D[near].min()]
    assert len(first) == 2 and set(r["label"][first].tolist()) == {0, 1}          # one core point of each block, exactly as far
    assert r["label"][mid] == r["label"][first.min()] and r["label"][first.min()] != r["label"][first.max()]
    lat = cr.dyadic_lattice()
    assert cr.cluster(lat, None, cr.LATTICE_PITCH, 1)["stats"]["clusters"] == len(lat)   # strict: a point one pitch away is no neighbour
    assert cr.cluster(lat, None, float(np.nextafter(cr.LATTICE_PITCH, 1.0)), 1)["stats"]["clusters"] == 1


@pytest.mark.parametrize("name", sorted(clouds()))
def test_adjacency_is_symmetric(name):
    p, radius, _ = clouds()[name]
    A = cr.adjacency(p, radius)
    assert (A == A.T).all() and A.diagonal().all()


@pytest.mark.parametrize("name", sorted(clouds()))
def test_min_pts_1_is_connected_components(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    p, radius, _ = clouds()[name]
    got = cr.cluster(p, None, radius, 1)
    nc, lab = csgraph.connected_components(sparse.csr_matrix(cr.adjacency(p, radius)), directed=False)
    assert nc == got["stats"]["clusters"] and got["core"].all() and got["stats"]["noise"] == 0
    # the same partition, numbered by the smallest index of a component
    first = np.full(nc, len(p))
    np.minimum.at(first, lab, np.arange(len(p)))
    rank = np.argsort(np.argsort(first))
    assert (rank[lab] == got["label"]).all()


@pytest.mark.parametrize("min_pts", [5, 17])
def test_blobs_equal_sklearn_on_core_points_and_noise(min_pts):
    skc = pytest.importorskip("sklearn.cluster")
    p, _ = cr.blobs_cloud()
    got = cr.cluster(p, None, cr.BLOBS_RADIUS, min_pts)
    # sklearn's neighbourhood is dist <= eps on its own distance computation: a radius between two representable distances of this cloud
    # makes the two predicates one (asserted: no pair lies within 1e-9 of the radius)
    D = np.sqrt(np.concatenate([cr.dist2_slab(p, a) for a in range(0, len(p), cr.SLAB)]))
    assert not (np.abs(D - cr.BLOBS_RADIUS) < 1e-9).any()
    db = skc.DBSCAN(eps=cr.BLOBS_RADIUS, min_samples=min_pts, algorithm="brute").fit(p)
    core = np.zeros(len(p), dtype=bool); core[db.core_sample_indices_] = True
    assert (core == (got["core"] == 1)).all()
    assert (db.labels_[core] == got["label"][core]).all()
    assert ((db.labels_ < 0) == (got["label"] < 0)).all()
    print("border points labelled differently:", int((db.labels_ != got["label"]).sum()))


def _abi_keep(lib, size, min_size, max_clusters):
    size = np.ascontiguousarray(size, dtype=np.int32)
    src = np.concatenate([size, np.zeros(1, np.int32)])
    keep = np.full(len(size) + 1, 7, dtype=np.uint8)
    st = lib.mvicp_cluster_keep_rule(len(size), src.ctypes.data_as(C.c_void_p), min_size, max_clusters, keep.ctypes.data_as(C.c_void_p))
    assert keep[-1] == 7
    return st, keep[:-1]


def test_keep_rule_through_the_abi(engine_lib):
    rng = np.random.Generator(np.random.PCG64(3))
    cases = [rng.integers(1, 6, size=40), rng.integers(1, 1000, size=17), np.array([5]), np.array([3, 3, 3, 3]), np.zeros(0, np.int32)]
    for size in cases:
        top = int(size.max()) if len(size) else 0
        for min_size in (0, 1, 3, top, top + 1):
            for max_clusters in (0, 1, 2, len(size), len(size) + 3):
                st, keep = _abi_keep(engine_lib, size, min_size, max_clusters)
                want = cr.keep_rule(size, min_size, max_clusters)
                assert st == 0 and keep.tobytes() == want.tobytes(), (size.tolist(), min_size, max_clusters)
                assert mvicp.cluster_keep_rule(size, min_size, max_clusters).tobytes() == want.tobytes()
    ties = np.array([4, 9, 4, 9, 4], dtype=np.int32)   # ranks: 1, 3 (size 9), then 0, 2, 4
    assert cr.keep_rule(ties, 0, 3).tolist() == [1, 1, 0, 1, 0] and _abi_keep(engine_lib, ties, 0, 3)[1].tolist() == [1, 1, 0, 1, 0]
    assert not cr.keep_rule(ties, 10, 0).any() and cr.keep_rule(ties, 0, 0).all() and cr.keep_rule(ties, 0, 9).all()
    assert cr.keep_rule(ties, 5, 3).tolist() == [0, 1, 0, 1, 0]
    # argument errors
    one = np.ones(2, dtype=np.int32); k = np.zeros(2, dtype=np.uint8)
    sp, kp = one.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)
    rule = engine_lib.mvicp_cluster_keep_rule
    assert rule(-1, sp, 0, 0, kp) == ERR_ARG and rule(2, sp, -1, 0, kp) == ERR_ARG and rule(2, sp, 0, -1, kp) == ERR_ARG
    assert rule(2, None, 0, 0, kp) == ERR_ARG and rule(2, sp, 0, 0, None) == ERR_ARG and rule(0, None, 0, 0, None) == ERR_ARG
    assert rule(2, sp, 0, 0, kp) == 0 and k.tolist() == [1, 1]


def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)


def test_argument_errors_need_no_gpu(engine_lib):
    clu, fetch, select, kept = engine_lib.mvicp_cluster, engine_lib.mvicp_cluster_fetch, engine_lib.mvicp_cluster_select, engine_lib.mvicp_cluster_fetch_kept
    assert clu(None, 0, 0.1, 4, None) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, None, 0, None) == ERR_ARG and select(None, 0, 0) == ERR_ARG and kept(None, 0, None, None, None, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for m in (0, -1, (1 << 30) + 1):
        assert clu(ctx, 0, 0.1, m, None) == ERR_ARG and b"min_pts" in engine_lib.mvicp_last_error(), m
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0):
        assert clu(ctx, 0, bad, 4, None) == ERR_ARG and b"radius" in engine_lib.mvicp_last_error(), bad
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range)
        assert clu(ctx, frame, 0.1, 4, None) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert select(ctx, -1, 0) == ERR_ARG and select(ctx, 0, -1) == ERR_ARG
    assert fake.raw == bytes(1 << 16)


def test_without_a_gpu_the_call_fails_loudly(engine_lib):
    """No device, no context, no clusters: mvicp_create refuses (there is no CPU path) and mvicp_cluster on the context it did not make
    reports an error instead of an answer.  With a device the same calls succeed on an empty context."""
    h = C.c_void_p()
    st = engine_lib.mvicp_create(0, C.byref(h))
    try:
        if st != 0:
            assert st == -2 and not h.value and b"no CPU fallback" in engine_lib.mvicp_last_error()
            with pytest.raises(mvicp.MvicpError):
                mvicp.Engine(0)
        assert engine_lib.mvicp_cluster(h, 0, 0.1, 4, None) == ERR_ARG   # a NULL context, or a context without frames
        assert len(engine_lib.mvicp_last_error()) > 0
    finally:
        if h.value:
            engine_lib.mvicp_destroy(h)


def test_overflow_rule():
    assert not cr.can_overflow(np.zeros((0, 3))) and not cr.can_overflow(np.array([[1e150, 0.0, 0.0]]))
    assert cr.can_overflow(np.array([[0.0, 0.0, 0.0], [1e154, 0.0, 0.0]]))
    with pytest.raises(OverflowError):
        cr.cluster(np.array([[0.0, 0.0, 0.0], [-1e154, 0.0, 0.0]]), None, 0.1, 1)
