"""Two-frame, one-edge linearization problems for the conditioning sweep (tests/test_gpu_lin_accuracy.py) and its CPU pre-check
(tests/test_xprec.py).  Test infrastructure only.

Base case: a source cloud of N points, spread 0.1 round its own origin; a relative transform (random rotation, translation of norm `tnorm`);
dst points q = R p + t + noise (sigma 2e-3) with random unit normals, both poses in general position; robust scale a = a_factor x the
residual noise.  One family varies at a time: tnorm, the offset W of both clouds from their frame origins, the unit of length, a_factor,
N (and option lin_chunk), exactly-zero residuals, the rotation angle."""
import numpy as np

from mvicp import synth

SPREAD, NOISE, N_BASE = 0.1, 2e-3, 20000
MIN_CLOUD = 64   # clouds are never smaller than this; fewer correspondences pick a subset of the points


def _unit(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def _pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R; P[:3, 3] = t
    return P


def make_case(name, seed=1, N=N_BASE, tnorm=0.0, W=0.0, unit=1.0, a_factor=1.0, angle=None, zero=False, chunk=0):
    """-> dict: src / dst clouds, dst normals, first / second (explicit lists), p / q / n (the gathered correspondences), poses [P_dst, P_src]
    (frame 0 = dst, frame 1 = src: the edge is 1 -> 0), a (float32), chunk (option lin_chunk, 0 = the library's choice), search_poses (the poses
    the searched route runs mvicp_correspond at: the poses themselves but for the zero family)."""
    rng = np.random.default_rng(seed)
    M = max(N, MIN_CLOUD)
    if zero:
        # exactly-zero residuals by construction: every coordinate a small multiple of 2^-10, rotations that permute the axes, normals with
        # three-bit components (not unit: the formulas never assume it) -> every product and sum below is exact in fp64 and in long double
        src = np.round(rng.normal(0, SPREAD, (M, 3)) * 1024) / 1024
        R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
        t = np.array([3.0, -1.5, 0.25])
        Pd = _pose(np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]]), np.array([0.5, 2.0, -1.0]))
        dst = src @ R.T + t
        nor = rng.integers(-4, 5, (M, 3)) / 4.0
        nor[np.all(nor == 0, axis=1)] = [0, 0, 1]
    else:
        src = (rng.normal(0, SPREAD, (M, 3)) + W * _unit(rng)) * unit
        R = synth.so3_exp(_unit(rng) * (rng.uniform(0.3, 2.5) if angle is None else angle))
        t = tnorm * unit * _unit(rng)
        Pd = _pose(synth.so3_exp(_unit(rng) * rng.uniform(0.3, 2.5)), rng.normal(0, 0.3, 3) * unit)
        dst = src @ R.T + t + rng.normal(0, NOISE * unit, (M, 3))
        nor = rng.normal(0, 1, (M, 3))
        nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    Ps = Pd @ _pose(R, t)
    search = None
    if zero:
        # poses to SEARCH at (the searched route): the dst frame moved by 2^-12 along world x, still exact.  Every query then finds its own match
        # at distance exactly 2^-12 (any other point of the 2^-10 lattice is at least 3 x 2^-12 away), so the search returns the identity list
        # with the scale 1.5 x 2^-12 > 0, where a search at the poses themselves would return the scale 0, for which the robust loss is undefined
        search = np.array([_pose(Pd[:3, :3], Pd[:3, 3] + [2.0 ** -12, 0, 0]), Ps])
    perm = rng.permutation(M)                       # dst is stored in another order than src
    dst_c, nor_c = np.empty_like(dst), np.empty_like(nor)
    dst_c[perm] = dst; nor_c[perm] = nor
    first = np.sort(rng.choice(M, N, replace=False)).astype(np.int32) if N < M else np.arange(M, dtype=np.int32)
    second = perm[first].astype(np.int32)
    a = np.float32(a_factor * NOISE * unit)
    return {"name": name, "src": np.ascontiguousarray(src), "dst": np.ascontiguousarray(dst_c), "nor": np.ascontiguousarray(nor_c),
            "first": first, "second": second, "poses": np.array([Pd, Ps]), "a": a, "chunk": chunk, "N": N,
            "search_poses": np.array([Pd, Ps]) if search is None else search}


def gathered(case, first=None, second=None):
    f = case["first"] if first is None else first
    s = case["second"] if second is None else second
    return case["src"][f], case["dst"][s], case["nor"][s]


# family -> list of make_case keyword sets.  Every N of the counts family and every chunk size appears at least once; odd N everywhere
# but 2 and 512 (16-byte pair loads, tail branch).
FAMILIES = {
    "t": [dict(tnorm=v) for v in (0.0, 1.0, 1e2, 1e4)],
    "W": [dict(W=v) for v in (0.0, 1e2, 1e4)],
    "unit": [dict(unit=v) for v in (1e-3, 1.0, 1e3)],
    "a": [dict(a_factor=v) for v in (1e-6, 1e-3, 1.0, 1e3, 1e6)],
    "count": [dict(N=1, chunk=512), dict(N=2, chunk=1024), dict(N=511, chunk=512), dict(N=512, chunk=512), dict(N=513, chunk=512),
              dict(N=513, chunk=4096), dict(N=20001, chunk=512), dict(N=20001, chunk=1024), dict(N=20001, chunk=4096), dict(N=20001, chunk=8192)],
    "zero": [dict(zero=True), dict(zero=True, N=513)],
    "angle": [dict(angle=v) for v in (0.0, 1e-9, 1e-4, np.pi - 1e-4, np.pi - 1e-9, np.pi)],
}
BIG = [dict(N=1000001, chunk=1024), dict(N=1000001, chunk=8192)]   # built once per module by the GPU sweep
# one searched route per family (identity list: the kernel reads p from the shared sorted source cloud); odd N
SEARCHED = {"t": dict(tnorm=1e2, N=20001), "W": dict(W=1e2, N=20001), "unit": dict(unit=1e3, N=20001), "a": dict(N=20001),
            "count": dict(N=513, chunk=512), "zero": dict(zero=True, N=20001), "angle": dict(angle=np.pi - 1e-4, N=20001)}


def case_name(family, kw):
    return family + ":" + ",".join("%s=%s" % (k, ("pi" + ("-%g" % (np.pi - v) if v < np.pi else "")) if k == "angle" and v > 3 else "%g" % v) for k, v in kw.items())


def all_cases():
    """-> [(family, name, kwargs)] of the explicit-list cases at base size (the 1 000 001-point cases are in BIG)"""
    out = []
    for fam, lst in FAMILIES.items():
        for i, kw in enumerate(lst):
            out.append((fam, case_name(fam, kw), dict(kw, seed=100 + 7 * len(out))))
    return out


def oracle_block(orc, case, plane, robust, first=None, second=None, a=None):
    f = case["first"] if first is None else first
    s = case["second"] if second is None else second
    return orc.edge_blocks([case["dst"], case["src"]], [case["nor"], case["nor"]], [1], [0], [(f, s)], [case["a"] if a is None else a],
                           case["poses"], plane, robust)[0]
