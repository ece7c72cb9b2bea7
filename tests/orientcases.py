"""The clouds and normals of the tests of mvicp_orient_normals (tests/test_orient_cpu.py, tests/test_gpu_orient.py): name -> (points,
normals, k, radius).  Normals come from the contract of mvicp_estimate_normals (normref) unless the case says otherwise, and every
point's sign is then scrambled at random, so a result that is consistent is the propagation's doing."""
import functools

import numpy as np

import normcases
import normref


def scramble(N, seed):
    s = np.where(np.random.default_rng(seed).integers(0, 2, len(N)) == 1, -1.0, 1.0)
    return np.ascontiguousarray(N * s[:, None])


def sphere(n=2000, seed=12):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1)[:, None])


def lattice(side=30, seed=4):
    """a flat side x side lattice in a shuffled index order, every normal (0, 0, 1): every weight is exactly 1"""
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float64) / 16
    g = g[np.random.default_rng(seed).permutation(len(g))]
    p = np.column_stack([g, np.zeros(len(g))])
    return np.ascontiguousarray(p), np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (len(p), 1)))


def helix(n=4096):
    """A helix whose spacing grows along it, so that with k = 2 every point's row is itself and its predecessor: the graph is one chain.
    The normals turn by ever smaller angles, so w grows along the chain, every point's best edge leads to its successor and the first
    round's hooks form one chain of n - 1 links: the pointer-jumping case."""
    t = np.cumsum(1.0 + 0.001 * np.arange(n)) * 0.01
    p = np.column_stack([np.cos(t), np.sin(t), 0.05 * t])
    ang = np.cumsum(0.3 / (1.0 + 0.01 * np.arange(n)))
    N = np.column_stack([np.cos(ang), np.sin(ang), np.zeros(n)])
    return np.ascontiguousarray(p), scramble(N, 9)


def islands(seed=8):
    """two clusters of 300 points and 12 far-off single points; with the radius 0.08 the single points have no neighbour at all"""
    rng = np.random.default_rng(seed)
    p = np.vstack([rng.normal(-0.5, 0.02, (300, 3)), rng.normal(0.5, 0.02, (300, 3)), rng.uniform(2.0, 9.0, (12, 3)) * [1, -1, 1]])
    p = p[rng.permutation(len(p))]
    return np.ascontiguousarray(p)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (p, N, k, radius)"""
    if name.startswith("blob"):
        p = normcases.placed("blob", 1.0, 0.0, 1200)
        return p, scramble(normref.normals(p, 16)["nrm"], 1), int(name[4:]), 0.0
    if name == "lattice":
        p, N = lattice()
        return p, N, 8, 0.0
    if name == "sphere":
        p = sphere()
        return p, scramble(normref.normals(p, 16)["nrm"], 2), 10, 0.0
    if name == "islands":
        p = islands()
        return p, scramble(normref.normals(p, 16, 0.08)["nrm"], 3), 10, 0.08
    if name in ("duplicates", "collinear"):
        p = normcases.duplicates() if name == "duplicates" else normcases.collinear()
        N = scramble(normref.normals(p, 16)["nrm"], 5)
        N[::7] = 0.0   # zero normals, as rows of fewer than 3 points leave them
        return p, np.ascontiguousarray(N), 10, 0.0
    if name == "helix":
        p, N = helix()
        return p, N, 2, 0.0
    if name == "small_far":
        p = normcases.placed("blob", 1e-3, 1e3, 1000)
        return p, scramble(normref.normals(p, 16)["nrm"], 6), 10, 0.0
    if name in ("n0", "n1", "n2"):
        n = int(name[1])
        return np.ascontiguousarray(np.array([[0.25, 0.5, -1.0], [0.5, 0.5, -1.0]])[:n]), np.ascontiguousarray(np.array([[0.0, 0.6, 0.8], [0.0, -0.6, -0.8]])[:n]), 2, 0.0
    raise KeyError(name)


CASES = ("blob2", "blob10", "blob64", "lattice", "sphere", "islands", "duplicates", "collinear", "helix", "small_far", "n0", "n1", "n2")


def votes():
    """The cloud of the mode tests, with the radius 0.3: three groups far from each other, every normal along +x or -x.
    A (x = 4 .. 4.4): after propagation its 5 normals point as point 0's does, +x, away from the origin: a VIEWPOINT vote at the origin flips it.
    B (x = -1, +1 about the point (0, 9, 0) -- two trees, for they are 2 apart): single points, s = 0 for neither.
    C (four points around (0, -9, 0) at x = -0.3, -0.1, 0.1, 0.3): one tree, two points on either side of the reference (0, -9, 0): a tie.
    -> (p, N)"""
    A = [[4.0 + 0.1 * i, 0.0, 0.0] for i in range(5)]
    B = [[-1.0, 9.0, 0.0], [1.0, 9.0, 0.0]]
    C = [[-0.3, -9.0, 0.0], [-0.1, -9.0, 0.0], [0.1, -9.0, 0.0], [0.3, -9.0, 0.0]]
    p = np.array(A + B + C)
    sg = np.array([1, -1, 1, 1, -1, 1, -1, -1, 1, 1, -1], dtype=np.float64)
    return np.ascontiguousarray(p), np.ascontiguousarray(np.outer(sg, [1.0, 0.0, 0.0]))
