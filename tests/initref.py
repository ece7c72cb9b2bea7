"""The contract of mvicp_poses_from_pairs (include/mvicp.h) in numpy and as a plain Python loop over scalars, the chain that
mvicp_coarse_pairs reduces to (matchref plus the gather), and the four-view fixture of tests/test_init_cpu.py, tests/test_gpu_coarse.py
and tests/test_gpu_init_driver.py.  fp64 throughout, every operation rounded on its own.

  usable       edge e iff count[e] >= min_count; pose[e] maps coordinates of frame src[e] into those of frame dst[e]
  forest       reached = {root}; among the usable edges with exactly one endpoint reached take the largest count, the lowest e among
               equals; repeat until none is left; then the lowest unreached frame starts the next component at the identity with
               parent = parent_edge = -1; component[i] numbers the components in the order they start
  composition  the new frame is dst[e]: pose_child = pose_parent T^-1, T^-1 = [R^T | -(R^T t)]; the new frame is src[e]:
               pose_child = pose_parent T; product: R = Ra Rb with entries (a0 b0 + a1 b1) + a2 b2, t = (Ra tb) + ta with a row times a
               vector as (r0 v0 + r1 v1) + r2 v2; bottom row 0 0 0 1; the root's pose is root_pose as given (None: the identity)
"""
import functools
import math

import numpy as np

import matchref as mr


# ---- poses from pairs
def _forest(n_frames, src, dst, count, min_count, root):
    """-> list of (child, parent, edge, child_is_dst, component) in the order frames are reached; parent = edge = -1 for a component's first"""
    if n_frames < 1 or not 0 <= root < n_frames or min_count < 0:
        raise ValueError("needs n_frames >= 1, a root in range and min_count >= 0")
    for s, d in zip(src, dst):
        if not (0 <= s < n_frames and 0 <= d < n_frames) or s == d:
            raise ValueError("an edge index out of range, or src == dst")
    reached = [False] * n_frames
    steps, comp, start = [], 0, root
    while start is not None:
        reached[start] = True
        steps.append((start, -1, -1, False, comp))
        while True:
            pick = -1
            for e in range(len(src)):
                if count[e] >= min_count and reached[src[e]] != reached[dst[e]] and (pick < 0 or count[e] > count[pick]):
                    pick = e
            if pick < 0:
                break
            child_is_dst = reached[src[pick]]
            child, parent = (dst[pick], src[pick]) if child_is_dst else (src[pick], dst[pick])
            reached[child] = True
            steps.append((child, parent, pick, child_is_dst, comp))
        comp += 1
        start = next((i for i in range(n_frames) if not reached[i]), None)
    return steps


def _finish(n_frames, steps, poses):
    parent = np.full(n_frames, -1, dtype=np.int32); pedge = np.full(n_frames, -1, dtype=np.int32); comp = np.zeros(n_frames, dtype=np.int32)
    for child, par, e, _, k in steps:
        parent[child], pedge[child], comp[child] = par, e, k
    return {"poses": np.ascontiguousarray(poses), "parent": parent, "parent_edge": pedge, "component": comp, "components": int(comp.max()) + 1}


def poses_from_pairs(n_frames, src, dst, count, pose, min_count=0, root=0, root_pose=None):
    """numpy form -> dict(poses (K,4,4), parent, parent_edge, component (K,) int32, components)"""
    src, dst, count = [int(v) for v in src], [int(v) for v in dst], [int(v) for v in count]
    T = np.asarray(pose, dtype=np.float64).reshape(-1, 4, 4)
    steps = _forest(n_frames, src, dst, count, min_count, root)
    poses = np.zeros((n_frames, 4, 4))

    def product(A, B):
        out = np.zeros((4, 4))
        Ra, Rb = A[:3, :3], B[:3, :3]
        out[:3, :3] = (Ra[:, 0][:, None] * Rb[0][None, :] + Ra[:, 1][:, None] * Rb[1][None, :]) + Ra[:, 2][:, None] * Rb[2][None, :]
        out[:3, 3] = ((Ra[:, 0] * B[0, 3] + Ra[:, 1] * B[1, 3]) + Ra[:, 2] * B[2, 3]) + A[:3, 3]
        out[3, 3] = 1.0
        return out

    def inverse(A):
        out = np.zeros((4, 4))
        Rt = A[:3, :3].T
        out[:3, :3] = Rt
        out[:3, 3] = -((Rt[:, 0] * A[0, 3] + Rt[:, 1] * A[1, 3]) + Rt[:, 2] * A[2, 3])
        out[3, 3] = 1.0
        return out

    for child, parent, e, child_is_dst, k in steps:
        if parent < 0:
            poses[child] = np.asarray(root_pose, dtype=np.float64).reshape(4, 4) if (k == 0 and root_pose is not None) else np.eye(4)
        else:
            poses[child] = product(poses[parent], inverse(T[e]) if child_is_dst else T[e])
    return _finish(n_frames, steps, poses)


def poses_from_pairs_loop(n_frames, src, dst, count, pose, min_count=0, root=0, root_pose=None):
    src, dst, count = [int(v) for v in src], [int(v) for v in dst], [int(v) for v in count]
    T = [[[float(x) for x in row] for row in M] for M in np.asarray(pose, dtype=np.float64).reshape(-1, 4, 4)]
    steps = _forest(n_frames, src, dst, count, min_count, root)
    eye = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    poses = [None] * n_frames

    def product(A, B):
        out = [[0.0] * 4 for _ in range(4)]
        for r in range(3):
            for c in range(3):
                out[r][c] = (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c]
            out[r][3] = ((A[r][0] * B[0][3] + A[r][1] * B[1][3]) + A[r][2] * B[2][3]) + A[r][3]
        out[3][3] = 1.0
        return out

    def inverse(A):
        out = [[0.0] * 4 for _ in range(4)]
        for r in range(3):
            for c in range(3):
                out[r][c] = A[c][r]
            out[r][3] = -((A[0][r] * A[0][3] + A[1][r] * A[1][3]) + A[2][r] * A[2][3])
        out[3][3] = 1.0
        return out

    for child, parent, e, child_is_dst, k in steps:
        if parent < 0:
            poses[child] = [[float(x) for x in row] for row in np.asarray(root_pose, dtype=np.float64).reshape(4, 4)] if (k == 0 and root_pose is not None) else eye
        else:
            poses[child] = product(poses[parent], inverse(T[e]) if child_is_dst else T[e])
    return _finish(n_frames, steps, np.array(poses, dtype=np.float64))


POSES_KEYS = ("poses", "parent", "parent_edge", "component", "components")


def rotation_angle(A, B):
    """the angle in radians between the rotations of two 4 x 4 poses"""
    from mvicp import synth
    return synth.pose_diff(np.asarray(A), np.asarray(B))[1]


def tree_path(parent, parent_edge, i):
    """the edges on the way from frame i up to the first frame of its component"""
    out = []
    while parent[i] >= 0:
        out.append(int(parent_edge[i]))
        i = int(parent[i])
    return out


# ---- the chain mvicp_coarse_pairs reduces to
def coarse_edge(desc_a, xyz_a, desc_b, xyz_b, mutual, ratio, H, seed, tau, edge_sim):
    """matchref's feature_match -> match_pairs -> the gather -> consensus (c >= 3)
    -> dict(pairs_n, best, count, accepted, pose (4,4), pairs (c,2) int32, flags (c,) uint8)"""
    mt = mr.feature_match(desc_a, desc_b)
    pairs = mr.match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], mutual, ratio)
    c = len(pairs)
    out = {"pairs_n": c, "best": -1, "count": 0, "accepted": 0, "pose": np.eye(4), "pairs": pairs, "flags": np.zeros(c, dtype=np.uint8)}
    if c >= 3:
        P, Q = np.ascontiguousarray(xyz_a[pairs[:, 0]]), np.ascontiguousarray(xyz_b[pairs[:, 1]])
        cons = mr.consensus(P, Q, H, seed, tau, edge_sim)
        out.update(best=cons["best"], count=cons["count"], accepted=cons["accepted"], pose=cons["pose"], flags=cons["flags"])
    return out


# ---- the four-view fixture
FIX_WINDOWS = ((0.0, 0.7), (0.2, 0.9), (0.4, 1.1), (0.6, 1.3))
FIX_H, FIX_EDGE_SIM, FIX_MAX_NN, FIX_MIN_COUNT = 8000, 0.9, 64, 20
FIX_EDGES = tuple((i, j) for i in range(4) for j in range(i + 1, 4))


def fix_seed(i, j):
    return 12345 + 4 * i + j


@functools.lru_cache(maxsize=None)
def fixture_clouds(n=1500):
    """Four views bumps(n, 100 + k, lo, hi) of one surface over the x windows FIX_WINDOWS.  View 0 stands at the identity, views 1 - 3 at
    (so3_exp(w), t) with w ~ U(-1, 1)^3 then t ~ U(-0.5, 0.5)^3 per view from PCG64(7); every cloud is stored in its own frame.  radius /
    spacing = the median distance from a point of view 0 to its 60th / nearest neighbour (n = 1500: 0.0991 and 0.01040), tau = 2 spacings.
    -> dict(xyz [4], nrm [4], gt (4,4,4) frame -> world, spacing, radius, tau)"""
    import knnref
    from mvicp import synth
    rng = np.random.Generator(np.random.PCG64(7))
    gt = np.tile(np.eye(4), (4, 1, 1))
    for k in range(1, 4):
        w = rng.uniform(-1.0, 1.0, size=3)
        t = rng.uniform(-0.5, 0.5, size=3)
        gt[k, :3, :3] = synth.so3_exp(w); gt[k, :3, 3] = t
    xyz, nrm = [], []
    for k, (lo, hi) in enumerate(FIX_WINDOWS):
        p, nn = mr.bumps(n, 100 + k, lo, hi)
        R, t = gt[k, :3, :3], gt[k, :3, 3]
        xyz.append(np.ascontiguousarray((p - t) @ R)); nrm.append(np.ascontiguousarray(nn @ R))   # (world -> frame: R^T (x - t))
    _, Ds = knnref.sorted_rows(xyz[0])   # (column 0 is the point itself)
    spacing = float(np.median(np.sqrt(Ds[:, 1])))
    radius = float(np.median(np.sqrt(Ds[:, min(60, n - 1)])))
    return {"xyz": xyz, "nrm": nrm, "gt": gt, "spacing": spacing, "radius": radius, "tau": 2.0 * spacing}


def relative_truth(gt, i, j):
    """the pose that maps coordinates of frame i into those of frame j"""
    return np.linalg.inv(gt[j]) @ gt[i]


@functools.lru_cache(maxsize=None)
def fixture_reference(n=1500):
    """The whole chain on the CPU for the fixture with n points per view: fpfhref descriptors -> coarse_edge per edge of FIX_EDGES
    (mutual, no ratio test, FIX_H hypotheses, seeds fix_seed(i, j)) -> poses_from_pairs(min_count = FIX_MIN_COUNT, root 0) over the
    consensus poses.  -> dict(desc [4], edges [E] of coarse_edge results, tree)"""
    import fpfhref
    cl = fixture_clouds(n)
    desc = [fpfhref.fpfh(cl["xyz"][k], cl["nrm"][k], cl["radius"], FIX_MAX_NN)["desc"] for k in range(4)]
    edges = [coarse_edge(desc[i], cl["xyz"][i], desc[j], cl["xyz"][j], True, 1.0, FIX_H, fix_seed(i, j), cl["tau"], FIX_EDGE_SIM) for i, j in FIX_EDGES]
    src, dst = [e[0] for e in FIX_EDGES], [e[1] for e in FIX_EDGES]
    tree = poses_from_pairs(4, src, dst, [e["count"] for e in edges], np.array([e["pose"] for e in edges]), FIX_MIN_COUNT, 0)
    return {"desc": desc, "edges": edges, "tree": tree}


def pose_error(pose, truth):
    """-> (rotation angle in degrees, |translation difference|)"""
    return mr.pose_error(pose, truth)
