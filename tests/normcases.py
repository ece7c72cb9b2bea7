"""The clouds of the tests of mvicp_estimate_normals (tests/test_normals_cpu.py, tests/test_gpu_estimate_normals.py)."""
import numpy as np

DIR = np.array([0.6, -0.48, 0.64])   # the direction the offset clouds are moved in (test_gpu_normals_accuracy)


def cloud(rng, n, kind):
    """the four kinds of test_gpu_normals_accuracy, extent ~ 1"""
    if kind == "blob":
        return rng.normal(0.0, 0.25, (n, 3))
    if kind == "plane":      # tilted, so the plane is not exact in fp64
        uv = rng.uniform(-1, 1, (n, 2))
        return uv @ np.array([[0.8, 0.1, 0.3], [-0.2, 0.9, 0.25]])
    if kind == "lattice":    # range-image grid: exact ties, with a smooth quantised depth
        side = int(np.ceil(n ** 0.5))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64) / side
        return np.column_stack([g, np.round(64 * 0.3 * np.sin(3 * g[:, 0]) * np.cos(2 * g[:, 1])) / 64])
    return np.vstack([rng.normal(-0.5, 0.02, (n // 2, 3)), rng.normal(0.5, 0.02, (n - n // 2, 3))])   # clusters


def placed(kind, scale, offset, n, seed=31):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((cloud(rng, n, kind) + offset * DIR) * scale)


def collinear(n=700, seed=6):
    """exactly collinear points along a dyadic direction: every coordinate exact"""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.choice(4096, n, replace=False)).astype(np.float64)
    return np.ascontiguousarray(np.outer(s, [0.25, -0.125, 0.5]) / 64 + [1.0, 2.0, -0.5])


def duplicates(sites=40, copies=20, seed=6):
    """`sites` random sites, each `copies` times, shuffled"""
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 0.1, (sites, 3))
    return np.ascontiguousarray(np.repeat(s, copies, axis=0)[rng.permutation(sites * copies)])


def constant_coordinate(axis, value, n=600, seed=5):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.2, 0.2, (n, 3))
    p[:, axis] = value
    return np.ascontiguousarray(p)
