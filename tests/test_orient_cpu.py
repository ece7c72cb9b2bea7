"""The contracts of mvicp_orient_normals and mvicp_signs_from_agreement on the CPU: tests/orientref.py's numpy form equals its scalar
Kruskal loop and an independent Prim on every case of tests/orientcases.py; what the propagation achieves on a sphere and on the four-view
fixture; the host rule mvicp_signs_from_agreement against both forms; the argument tables."""
import ctypes as C
import heapq

import numpy as np
import pytest

import initref
import mvicp
import normref
import orientcases as oc
import orientref as oref
from mvicp import lib as L


def prim(p, N, rows):
    """An independent maximum spanning forest: Prim with a heap over the key (-w, min, max), a new tree from the lowest unreached index.
    -> (set of forest edges, comp, x)"""
    n = len(p)
    a, b = oref.graph_edges(rows, n)
    adj = [[] for _ in range(n)]
    for u, v in zip(a.tolist(), b.tolist()):
        d = (N[u, 0] * N[v, 0] + N[u, 1] * N[v, 1]) + N[u, 2] * N[v, 2]
        adj[u].append((-abs(d), u, v, v, int(d < 0))); adj[v].append((-abs(d), u, v, u, int(d < 0)))
    comp, x, forest = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint8), set()
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = s
        heap = list(adj[s])
        heapq.heapify(heap)
        while heap:
            _, u, v, to, f = heapq.heappop(heap)
            if comp[to] >= 0:
                continue
            frm = u if to == v else v
            comp[to] = s; x[to] = x[frm] ^ f
            forest.add((u, v))
            for item in adj[to]:
                if comp[item[3]] < 0:
                    heapq.heappush(heap, item)
    return forest, comp, x


@pytest.mark.parametrize("name", oc.CASES)
def test_numpy_form_equals_the_scalar_loop_and_an_independent_prim(name):
    p, N, k, radius = oc.case(name)
    a = oref.orient(p, N, k, radius)
    b = oref.orient_loop(p, N, k, radius, rows=a["knn"])
    assert oref.same(a, b)
    forest, comp, x = prim(p, N, a["knn"])
    assert forest == set(a["forest"]) and comp.tobytes() == a["comp"].tobytes() and x.tobytes() == a["flip"].tobytes()
    assert len(a["forest"]) == len(p) - a["components"]
    for mode, ref in ((oref.VIEWPOINT, None), (oref.VIEWPOINT, (0.3, -0.2, 5.0)), (oref.DIRECTION, (0.6, -0.48, 0.64))):
        assert oref.same(oref.orient(p, N, k, radius, mode, ref, rows=a["knn"]), oref.orient_loop(p, N, k, radius, mode, ref, rows=a["knn"]))


def test_case_shapes():
    """what the cases are there for"""
    res = {name: oref.orient(*oc.case(name)) for name in ("lattice", "islands", "helix", "duplicates", "collinear")}
    p, N, k, radius = oc.case("lattice")
    assert (N == [0.0, 0.0, 1.0]).all() and res["lattice"]["components"] == 1 and not res["lattice"]["flip"].any()
    assert res["islands"]["components"] == 2 + 12 and (np.bincount(res["islands"]["comp"]) == 1).sum() == 12
    p, N, k, radius = oc.case("helix")
    idx = res["helix"]["knn"]["idx"]
    assert k == 2 and (idx[1:, 1] == np.arange(len(p) - 1)).all() and res["helix"]["components"] == 1
    d = np.abs((N[:-1] * N[1:]).sum(1))
    assert (np.diff(d) > 0).all()      # every point's heavier edge leads to its successor: the first round's hooks are one chain
    for name in ("duplicates", "collinear"):
        assert (oc.case(name)[1][::7] == 0).all()


def test_sphere_ends_on_one_side():
    p, N, k, radius = oc.case("sphere")
    assert len(p) == 2000 and k == 10
    before = np.sign((N * p).sum(1))
    assert 800 < (before > 0).sum() < 1200                      # scrambled
    r = oref.orient(p, N, k, radius)
    assert r["components"] == 1
    side = np.sign((r["nrm"] * p).sum(1))
    assert (side == side[0]).all() and side[0] != 0            # p is the radial direction of the unit sphere
    out = oref.orient(p, N, k, radius, oref.VIEWPOINT, None, rows=r["knn"])     # the centre as viewpoint: everything points inwards
    assert ((out["nrm"] * p).sum(1) < 0).all()
    out = oref.orient(p, N, k, radius, oref.VIEWPOINT, (0.0, 0.0, 50.0), rows=r["knn"])   # a viewpoint outside sees the near half: a tie within noise, but consistent
    side = np.sign((out["nrm"] * p).sum(1))
    assert (side == side[0]).all()


@pytest.mark.parametrize("k", [8, 10, 16])
def test_fixture_views_are_one_component_on_one_side(k):
    cl = initref.fixture_clouds()
    sides = []
    for v in range(4):
        p = cl["xyz"][v]
        est = normref.normals(p, 16)["nrm"]
        r = oref.orient(p, est, k)
        assert r["components"] == 1
        side = np.sign((r["nrm"] * cl["nrm"][v]).sum(1))
        assert (side == side[0]).all() and side[0] != 0
        sides.append(int(side[0]))
    assert sides == [-1, 1, -1, 1]      # views 0 and 2 end opposite to the fixture's normals: the step between the clouds is needed


# ---- the host rule

def both(K, src, dst, pos, neg, min_count=0):
    a, b = oref.signs(K, src, dst, pos, neg, min_count), oref.signs_loop(K, src, dst, pos, neg, min_count)
    got = mvicp.signs_from_agreement(K, src, dst, pos, neg, min_count)
    assert oref.same_signs(a, b) and oref.same_signs(a, got), (a, b, got)
    return got


def test_signs_chain():
    got = both(5, [0, 1, 2, 3], [1, 2, 3, 4], [10, 2, 9, 0], [1, 30, 3, 7])
    assert got["components"] == 1 and got["flip"].tolist() == [0, 0, 1, 1, 0] and got["component"].tolist() == [0] * 5
    got = both(3, [2, 1], [1, 0], [0, 0], [5, 5])      # reversed edges: the direction does not matter
    assert got["flip"].tolist() == [0, 1, 0]


def test_signs_cycle_with_one_inconsistent_edge():
    # 0-1 agree (90), 1-2 disagree (80), 2-0 claims agreement (weakest, 12): it would make the cycle inconsistent and is left out
    got = both(3, [0, 1, 2], [1, 2, 0], [100, 10, 20], [10, 90, 8])
    assert got["components"] == 1 and got["flip"].tolist() == [0, 0, 1]
    # the same with the weak edge made the strongest: now the 1-2 edge (weakest) is the one left out
    got = both(3, [0, 1, 2], [1, 2, 0], [100, 10, 200], [10, 60, 8])
    assert got["flip"].tolist() == [0, 0, 0]
    # equal margins: the lower edge index first
    got = both(3, [0, 1, 2], [1, 2, 0], [0, 0, 50], [50, 50, 0])
    assert got["flip"].tolist() == [0, 1, 0]


def test_signs_components_and_min_count():
    src, dst, pos, neg = [0, 1, 3, 4, 2], [1, 2, 4, 5, 3], [9, 0, 0, 8, 5], [0, 9, 7, 0, 5]
    got = both(7, src, dst, pos, neg)                  # edge 4 is a tie: unusable; frame 6 has no edge
    assert got["components"] == 3 and got["component"].tolist() == [0, 0, 0, 3, 3, 3, 6] and got["flip"].tolist() == [0, 0, 1, 0, 1, 1, 0]
    got = both(7, src, dst, pos, neg, 9)               # the cut: edges 2 and 3 fall below 9 pairs
    assert got["components"] == 5 and got["component"].tolist() == [0, 0, 0, 3, 4, 5, 6] and got["flip"].tolist() == [0, 0, 1, 0, 0, 0, 0]
    got = both(2, [], [], [], [])
    assert got["components"] == 2
    rng = np.random.default_rng(3)
    for _ in range(40):
        K, E = int(rng.integers(1, 9)), int(rng.integers(0, 20))
        s = rng.integers(0, K, E); d = (s + rng.integers(1, max(K, 2), E)) % K
        ok = s != d
        both(K, s[ok], d[ok], rng.integers(0, 6, E)[ok], rng.integers(0, 6, E)[ok], int(rng.integers(0, 5)))


def test_argument_tables():
    lib = L.load_library()
    i4 = lambda *v: np.array(v, dtype=np.int32)
    flip, comp = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.int32)
    fp = flip.ctypes.data_as(C.POINTER(C.c_ubyte))

    def call(K, E, src, dst, pos, neg, mc, f=fp):
        return lib.mvicp_signs_from_agreement(K, E, L._ip(src), L._ip(dst), L._ip(pos), L._ip(neg), mc, f, L._ip(comp))

    good = (i4(0, 1), i4(1, 2), i4(3, 0), i4(0, 3))
    assert call(3, 2, *good, 0) == 1
    assert call(0, 2, *good, 0) == -1 and call(3, -1, *good, 0) == -1 and call(3, 2, *good, -1) == -1 and call(3, 2, *good, 0, None) == -1
    assert call(3, 2, i4(0, 3), *good[1:], 0) == -1 and call(3, 2, i4(0, 2), *good[1:], 0) == -1 and call(3, 2, i4(0, -1), *good[1:], 0) == -1
    assert call(3, 2, good[0], good[1], i4(3, -1), good[3], 0) == -1
    assert lib.mvicp_signs_from_agreement(3, 2, None, L._ip(good[1]), L._ip(good[2]), L._ip(good[3]), 0, fp, None) == -1
    assert lib.mvicp_signs_from_agreement(3, 0, None, None, None, None, 0, fp, None) == 3
    # the device calls refuse a null context before anything else
    assert lib.mvicp_orient_normals(None, 0, 0, 10, 0.0, 0, None) == -1 and lib.mvicp_orient_fetch(None, 0, None, None, None) == -1
    assert lib.mvicp_orient_adopt(None) == -1 and lib.mvicp_negate_normals(None, 0) == -1 and lib.mvicp_normal_agreement(None, None, None, None) == -1
    # the reference refuses what the library refuses
    p, N = np.zeros((3, 3)), np.ones((3, 3))
    for k, radius, mode, ref in ((1, 0.0, 0, None), (65, 0.0, 0, None), (10, float("nan"), 0, None), (10, float("inf"), 0, None), (10, 0.0, 3, None),
                                 (10, 0.0, -1, None), (10, 0.0, 2, None), (10, 0.0, 1, (0.0, float("nan"), 0.0)), (10, 0.0, 2, (float("inf"), 0.0, 0.0))):
        with pytest.raises(ValueError):
            oref.orient(p, N, k, radius, mode, ref)
        with pytest.raises(ValueError):
            oref.orient_loop(p, N, k, radius, mode, ref)
    bad = np.array([[1.0, 0.0, 0.0], [float("inf"), 0.0, 0.0], [0.0, 1.0, 0.0]])
    q = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    for fn in (oref.orient, oref.orient_loop):
        with pytest.raises(ValueError):
            fn(q, bad, 3)
