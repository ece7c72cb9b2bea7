"""mvicp_poses_from_pairs (a pure host function: no GPU) against its numpy and scalar-loop statements in tests/initref.py, byte for
byte, and the four-view fixture end to end on the CPU: fpfhref descriptors -> matchref matching and consensus per edge -> the spanning
tree and the composed poses.  What a case must contain (a tie in the counts, an edge walked backwards, a second component) is asserted on
the reference alone, so no case can pass trivially."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import initref as ir
import mvicp
from mvicp import lib as L
from mvicp import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def same(a, b, what):
    for key in ir.POSES_KEYS:
        x, y = a[key], b[key]
        if key == "components":
            assert int(x) == int(y), (what, key, x, y)
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, key, x, y)


def random_pose(rng, angle=1.0, shift=1.0):
    T = np.eye(4)
    T[:3, :3] = synth.so3_exp(rng.uniform(-angle, angle, size=3)); T[:3, 3] = rng.uniform(-shift, shift, size=3)
    return T


def random_graph(rng, K, extra, connected=True):
    """a random spanning tree (when connected) plus `extra` more edges, each in a random direction"""
    edges = []
    if connected:
        order = rng.permutation(K)
        for k in range(1, K):
            a, b = int(order[k]), int(order[rng.integers(0, k)])
            edges.append((a, b) if rng.integers(0, 2) else (b, a))
    for _ in range(extra):
        a, b = rng.choice(K, size=2, replace=False)
        edges.append((int(a), int(b)))
    return edges


def check_all_forms(K, edges, count, pose, min_count=0, root=0, root_pose=None, what=""):
    src, dst = [e[0] for e in edges], [e[1] for e in edges]
    want = ir.poses_from_pairs(K, src, dst, count, pose, min_count, root, root_pose)
    loop = ir.poses_from_pairs_loop(K, src, dst, count, pose, min_count, root, root_pose)
    same(want, loop, (what, "numpy vs loop"))
    got = mvicp.poses_from_pairs(K, src, dst, count, pose, min_count, root, root_pose)
    same(got, want, (what, "library vs numpy"))
    return got


@pytest.mark.parametrize("seed", range(6))
def test_equals_the_reference_on_random_graphs(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    K = int(rng.integers(2, 12))
    edges = random_graph(rng, K, extra=int(rng.integers(0, 2 * K)), connected=bool(seed % 2))
    count = rng.integers(0, 6, size=len(edges))   # (few distinct values: ties are the rule)
    pose = np.array([random_pose(rng) for _ in edges]).reshape(-1, 4, 4)
    for min_count in (0, 3):
        for root in (0, K - 1):
            check_all_forms(K, edges, count, pose, min_count, root, None if root == 0 else random_pose(rng), what=(seed, min_count, root))


def test_ground_truth_relative_poses_return_the_ground_truth():
    """pose[e] = inv(gt[dst]) gt[src] maps coordinates of src into those of dst: with the root at gt[root] every frame comes back to its
    ground truth, whichever way the tree walks the edges.  This pins the convention.  1e-12: a path of at most K - 1 = 8 products of
    rotations with unit norm and translations below 3 accumulates a few ulps of 3 per step, about 10 x 8 x 3 x 2.2e-16 < 1e-13."""
    rng = np.random.Generator(np.random.PCG64(42))
    K = 9
    gt = np.array([random_pose(rng) for _ in range(K)])
    edges = random_graph(rng, K, extra=6)
    pose = np.array([np.linalg.inv(gt[d]) @ gt[s] for s, d in edges])
    count = rng.integers(1, 100, size=len(edges))
    for root in (0, 4):
        got = check_all_forms(K, edges, count, pose, 0, root, gt[root], what=("gt", root))
        assert got["components"] == 1 and (got["component"] == 0).all()
        assert np.abs(got["poses"] - gt).max() < 1e-12, np.abs(got["poses"] - gt).max()
        walked_backwards = [k for k in range(K) if got["parent"][k] >= 0 and edges[got["parent_edge"][k]][0] == k]
        walked_forwards = [k for k in range(K) if got["parent"][k] >= 0 and edges[got["parent_edge"][k]][1] == k]
        assert walked_backwards and walked_forwards   # (both compositions occur)


def test_ties_in_count_go_to_the_lowest_edge():
    rng = np.random.Generator(np.random.PCG64(1))
    edges = [(0, 1), (0, 2), (1, 2), (0, 1)]   # a triangle, and edge 3 repeats edge 0 with another pose
    pose = np.array([random_pose(rng) for _ in edges])
    got = check_all_forms(3, edges, [5, 5, 5, 5], pose, what="ties")
    assert got["parent"].tolist() == [-1, 0, 0] and got["parent_edge"].tolist() == [-1, 0, 1]
    got = check_all_forms(3, edges, [5, 5, 6, 6], pose, what="ties 2")   # edge 3 first (the largest reachable), then edge 2
    assert got["parent"].tolist() == [-1, 0, 1] and got["parent_edge"].tolist() == [-1, 3, 2]


def test_an_edge_given_in_the_reverse_direction():
    rng = np.random.Generator(np.random.PCG64(2))
    T = random_pose(rng)
    fwd = check_all_forms(2, [(0, 1)], [9], T[None], what="forward")     # frame 1 is dst: pose_1 = T^-1
    rev = check_all_forms(2, [(1, 0)], [9], T[None], what="reverse")     # frame 1 is src: pose_1 = T
    assert rev["poses"][1].tobytes() == T.tobytes()
    assert np.abs(fwd["poses"][1] @ T - np.eye(4)).max() < 1e-14
    assert fwd["parent"].tolist() == rev["parent"].tolist() == [-1, 0]


def test_min_count_splits_the_graph():
    rng = np.random.Generator(np.random.PCG64(3))
    edges = [(0, 1), (1, 2), (2, 3), (3, 4)]
    pose = np.array([random_pose(rng) for _ in edges])
    got = check_all_forms(5, edges, [30, 4, 25, 21], pose, min_count=20, what="split")
    assert got["components"] == 2 and got["component"].tolist() == [0, 0, 1, 1, 1]
    assert got["parent"].tolist() == [-1, 0, -1, 2, 3] and got["parent_edge"].tolist() == [-1, 0, -1, 2, 3]
    assert got["poses"][2].tobytes() == np.eye(4).tobytes()
    got = check_all_forms(5, edges, [30, 4, 25, 21], pose, min_count=20, root=3, what="split, root 3")
    assert got["component"].tolist() == [1, 1, 0, 0, 0] and got["parent"].tolist() == [-1, 0, 3, -1, 3]
    got = check_all_forms(5, edges, [30, 4, 25, 21], pose, min_count=31, what="nothing usable")
    assert got["components"] == 5 and got["component"].tolist() == [0, 1, 2, 3, 4] and (got["parent"] == -1).all()


def test_one_frame_and_no_edges():
    rng = np.random.Generator(np.random.PCG64(4))
    T = random_pose(rng)
    got = check_all_forms(1, [], [], np.zeros((0, 4, 4)), what="K = 1")
    assert got["components"] == 1 and got["poses"][0].tobytes() == np.eye(4).tobytes()
    got = check_all_forms(3, [], [], np.zeros((0, 4, 4)), root=1, root_pose=T, what="E = 0")
    assert got["components"] == 3 and got["component"].tolist() == [1, 0, 2]
    assert got["poses"][1].tobytes() == T.tobytes() and got["poses"][0].tobytes() == np.eye(4).tobytes()


def test_every_argument_error(engine_lib):
    f = engine_lib.mvicp_poses_from_pairs
    src, dst, count = (np.array(v, dtype=np.int32) for v in ([0, 1], [1, 2], [5, 5]))
    pose = np.tile(np.eye(4).reshape(1, 16), (2, 1))
    out = np.zeros((3, 16)); par = np.zeros(3, dtype=np.int32)
    ip, dp = L._ip, L._dp

    def call(K=3, E=2, s=src, d=dst, c=count, p=pose, min_count=0, root=0, o=out):
        return f(K, E, None if s is None else ip(s), None if d is None else ip(d), None if c is None else ip(c), None if p is None else dp(p),
                 min_count, root, None, None if o is None else dp(o), ip(par), None, None)

    assert call() == 1   # (the optional outputs may be NULL)
    for kw in (dict(s=None), dict(d=None), dict(c=None), dict(p=None), dict(o=None), dict(K=0), dict(E=-1), dict(root=-1), dict(root=3), dict(min_count=-1),
               dict(s=np.array([0, 3], dtype=np.int32)), dict(d=np.array([1, -1], dtype=np.int32)), dict(s=np.array([0, 2], dtype=np.int32))):
        assert call(**kw) == ERR_ARG, kw
        assert engine_lib.mvicp_last_error()
    assert call(E=0, s=None, d=None, c=None, p=None) == 3   # (no edges: no edge arrays needed)


def test_composed_rotation_error_is_bounded_by_the_path():
    """The triangle inequality on SO(3): the angle between a composed pose and the truth is at most the sum of the angles between each
    edge of its tree path and that edge's truth, + 1e-9 for the rounding of the products and of the angle itself."""
    rng = np.random.Generator(np.random.PCG64(5))
    K = 8
    gt = np.array([random_pose(rng) for _ in range(K)])
    gt[0] = np.eye(4)
    edges = random_graph(rng, K, extra=5)
    noisy = np.array([np.linalg.inv(gt[d]) @ gt[s] @ random_pose(rng, 0.03, 0.01) for s, d in edges])
    got = check_all_forms(K, edges, rng.integers(1, 50, size=len(edges)), noisy, what="noisy")
    edge_err = [ir.rotation_angle(noisy[e], np.linalg.inv(gt[d]) @ gt[s]) for e, (s, d) in enumerate(edges)]
    assert max(edge_err) > 1e-3
    for k in range(1, K):
        path = ir.tree_path(got["parent"], got["parent_edge"], k)
        assert ir.rotation_angle(got["poses"][k], gt[k]) <= sum(edge_err[e] for e in path) + 1e-9, (k, path)


def test_fixture_end_to_end_on_the_cpu():
    """Measured with matchref and fpfhref on the CPU (pairs / accepted / inliers, then the consensus pose against the truth as rotation
    angle and |translation difference| in spacings):
        (0,1) 354 / 120 / 43  0.50 deg 1.08      (0,2) 327 / 68 / 39   1.71 deg 1.52     (0,3) 247 / 12 / 5  176 deg
        (1,2) 388 / 316 / 84  0.96 deg 2.23      (1,3) 283 / 101 / 37  1.85 deg 3.02     (2,3) 350 / 333 / 65  1.61 deg 2.05
    With min_count = 20 the tree from root 0 is the chain 0 - 1 - 2 - 3 and edge (0,3) is dropped; the composed poses are 0.50 deg / 1.48,
    1.14 deg / 2.76 and 0.51 deg / 1.20 spacings from the truth.  Every tree edge meets the bound of tests/test_match_cpu.py, 3 deg and 3
    spacings; the composed rotations meet the triangle inequality."""
    cl, ref = ir.fixture_clouds(), ir.fixture_reference()
    assert abs(cl["radius"] - 0.0991) < 5e-5 and abs(cl["spacing"] - 0.01040) < 5e-6
    table = {e: (r["pairs_n"], r["accepted"], r["count"]) for e, r in zip(ir.FIX_EDGES, ref["edges"])}
    print(table)
    assert table == {(0, 1): (354, 120, 43), (0, 2): (327, 68, 39), (0, 3): (247, 12, 5), (1, 2): (388, 316, 84), (1, 3): (283, 101, 37),
                     (2, 3): (350, 333, 65)}
    tree = ref["tree"]
    assert tree["components"] == 1 and tree["parent"].tolist() == [-1, 0, 1, 2]
    assert [ir.FIX_EDGES[e] for e in tree["parent_edge"][1:]] == [(0, 1), (1, 2), (2, 3)]
    assert ref["edges"][ir.FIX_EDGES.index((0, 3))]["count"] < ir.FIX_MIN_COUNT
    src, dst = [e[0] for e in ir.FIX_EDGES], [e[1] for e in ir.FIX_EDGES]
    got = mvicp.poses_from_pairs(4, src, dst, [r["count"] for r in ref["edges"]], np.array([r["pose"] for r in ref["edges"]]), ir.FIX_MIN_COUNT, 0)
    same(got, tree, "fixture tree")
    edge_rot = {}
    for e in tree["parent_edge"][1:]:
        i, j = ir.FIX_EDGES[e]
        deg, dt = ir.pose_error(ref["edges"][e]["pose"], ir.relative_truth(cl["gt"], i, j))
        print("edge", (i, j), "deg", deg, "spacings", dt / cl["spacing"])
        assert deg < 3.0 and dt < 3.0 * cl["spacing"]
        edge_rot[int(e)] = math.radians(deg)
    for k in range(1, 4):
        deg, dt = ir.pose_error(tree["poses"][k], cl["gt"][k])
        print("frame", k, "deg", deg, "spacings", dt / cl["spacing"])
        assert math.radians(deg) <= sum(edge_rot[e] for e in ir.tree_path(tree["parent"], tree["parent_edge"], k)) + 1e-9


def test_header_and_binding_agree(tmp_path):
    assert C.sizeof(L.CoarseEdge) == 144 and L.CoarseEdge.pose.offset == 16
    src = tmp_path / "coarse_c.c"
    src.write_text('#include "mvicp.h"\n#include <stddef.h>\n'
                   'typedef char edge_is_144_bytes[(sizeof(mvicp_coarse_edge) == 144 && offsetof(mvicp_coarse_edge, pairs) == 0 && '
                   'offsetof(mvicp_coarse_edge, best) == 4 && offsetof(mvicp_coarse_edge, count) == 8 && offsetof(mvicp_coarse_edge, accepted) == 12 && '
                   'offsetof(mvicp_coarse_edge, pose) == 16) ? 1 : -1];\n'
                   'long long use(mvicp_ctx* c, mvicp_coarse_edge* r) { return mvicp_coarse_pairs(c, 0, 0, 0, 1, 33, 0, 0, 0, 0, 1, 1.0, 1, 1.0, 0.9, r) + '
                   'mvicp_coarse_pairs_fetch(c, 0, 0, 0, 0) + mvicp_poses_from_pairs(1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "coarse_c.o")])
    for name in ("mvicp_coarse_pairs", "mvicp_coarse_pairs_fetch", "mvicp_poses_from_pairs"):
        assert name in L.SYMBOLS and hasattr(mvicp.load_library(), name)
    assert [f for f, _ in L.CoarseEdge._fields_] == ["pairs", "best", "count", "accepted", "pose"]
