"""The contract of mvicp_outlier_filter (include/mvicp.h) in numpy: brute-force n x n distances in the metric's operation order, the k+1
smallest values per point, Python integers for the sums of the statistical rule.  `outlier_filter_loop` is the same statement as a plain
Python loop over scalars; `threshold` is the rule of mvicp_outlier_threshold."""
import math

import numpy as np


def dist2_matrix(p):
    """(d0 d0 + d1 d1) + d2 d2 for all pairs, every operation rounded on its own (numpy never contracts to fma)."""
    d = p[:, None, :] - p[None, :, :]
    return (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]


def k_distances(p, k):
    """(mdist, kd2) per point; rows are done in slabs so that a 5000-point cloud needs no 5000 x 5000 x 3 temporary."""
    n = len(p)
    mdist, kd2 = np.zeros(n), np.zeros(n)
    for a in range(0, n, 512):
        d = p[a:a + 512, None, :] - p[None, :, :]
        D = np.sort((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2], axis=1)[:, :k + 1]
        s = np.zeros(len(D))
        for t in range(1, k + 1):
            s = s + np.sqrt(D[:, t])
        mdist[a:a + 512] = s / float(k)
        kd2[a:a + 512] = D[:, k]
    return mdist, kd2


def q_exponent(mmax):
    """The integer q with 2^30 <= mmax 2^q < 2^31 (mmax > 0)."""
    _, ex = math.frexp(mmax)   # mmax = m 2^ex, m in [0.5, 1)
    return 31 - ex


def threshold(n, s1, s2, std_ratio):
    """T of the statistical rule from exact integer sums: Python's float(int) is round-to-nearest-even."""
    mean = float(s1) / float(n)
    var = (float(n * s2 - s1 * s1) / float(n)) / (float(n) - 1.0)
    return mean + std_ratio * math.sqrt(var)


def outlier_filter(p, nrm, k, std_ratio, radius):
    p = np.ascontiguousarray(p, dtype=np.float64)
    n = len(p)
    stats = {"n": n, "kept": 0, "q_exp": 0, "s1": 0, "s2": 0, "s2_hi": 0, "s2_lo": 0, "T": 0.0, "threshold": 0.0, "has_normals": int(nrm is not None)}
    if n == 0:
        return {"xyz": p.reshape(0, 3), "nrm": None if nrm is None else np.zeros((0, 3)), "idx": np.zeros(0, np.int32), "mdist": np.zeros(0),
                "kd2": np.zeros(0), "stats": stats}
    if not 1 <= k <= 32 or n <= k:
        raise ValueError("needs 1 <= k <= 32 and n > k")
    mdist, kd2 = k_distances(p, k)
    keep = np.ones(n, dtype=bool)
    if radius > 0:
        keep &= np.sqrt(kd2) < radius
    if std_ratio >= 0 and mdist.max() > 0:
        q = q_exponent(float(mdist.max()))
        M = np.floor(np.ldexp(mdist, q)).astype(np.int64)
        assert (1 << 30) <= int(M.max()) < (1 << 31)
        s1 = sum(int(m) for m in M)
        s2 = sum(int(m) * int(m) for m in M)
        T = threshold(n, s1, s2, std_ratio)
        keep &= M.astype(np.float64) <= T
        stats.update(q_exp=q, s1=s1, s2=s2, s2_hi=s2 >> 64, s2_lo=s2 & ((1 << 64) - 1), T=T, threshold=math.ldexp(T, -q))
    idx = np.flatnonzero(keep).astype(np.int32)
    stats["kept"] = len(idx)
    return {"xyz": p[idx], "nrm": None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float64)[idx], "idx": idx, "mdist": mdist,
            "kd2": kd2, "stats": stats}


def outlier_filter_loop(p, nrm, k, std_ratio, radius):
    """The same contract, one scalar operation at a time."""
    n = len(p)
    mdist, kd2 = [], []
    for i in range(n):
        ds = []
        for j in range(n):
            d0, d1, d2 = float(p[i][0]) - float(p[j][0]), float(p[i][1]) - float(p[j][1]), float(p[i][2]) - float(p[j][2])
            ds.append((d0 * d0 + d1 * d1) + d2 * d2)
        ds.sort()
        s = 0.0
        for t in range(1, k + 1):
            s = s + math.sqrt(ds[t])
        mdist.append(s / float(k))
        kd2.append(ds[k])
    mmax = max(mdist)
    stat = std_ratio >= 0 and mmax > 0
    q = s1 = s2 = 0
    T = 0.0
    if stat:
        q = q_exponent(mmax)
        M = [int(math.floor(math.ldexp(m, q))) for m in mdist]
        s1, s2 = sum(M), sum(m * m for m in M)
        T = threshold(n, s1, s2, std_ratio)
    idx = [i for i in range(n) if (not stat or float(M[i]) <= T) and (not radius > 0 or math.sqrt(kd2[i]) < radius)]
    idx = np.array(idx, dtype=np.int32)
    stats = {"n": n, "kept": len(idx), "q_exp": q, "s1": s1, "s2": s2, "s2_hi": s2 >> 64, "s2_lo": s2 & ((1 << 64) - 1), "T": T,
             "threshold": math.ldexp(T, -q), "has_normals": int(nrm is not None)}
    return {"xyz": np.asarray(p)[idx], "nrm": None if nrm is None else np.asarray(nrm)[idx], "idx": idx, "mdist": np.array(mdist),
            "kd2": np.array(kd2), "stats": stats}


def same(a, b):
    """Byte equality of two results, stats included."""
    for key in ("xyz", "nrm", "idx", "mdist", "kd2"):
        if (a[key] is None) != (b[key] is None):
            return False
        if a[key] is not None and (a[key].shape != b[key].shape or np.ascontiguousarray(a[key]).tobytes() != np.ascontiguousarray(b[key]).tobytes()):
            return False
    sa, sb = a["stats"], b["stats"]
    if any(int(sa[key]) != int(sb[key]) for key in ("n", "kept", "q_exp", "s1", "s2_hi", "s2_lo", "has_normals")):
        return False
    return all(np.float64(sa[key]).tobytes() == np.float64(sb[key]).tobytes() for key in ("T", "threshold"))


# ---- the clouds of the tests
def sheet_cloud(n, seed):
    """A thin sheet (xy uniform in [-0.4, 0.6]^2, z noise sigma = 2 mm) with ceil(n / 50) planted points 5 - 30 cm off it, at random
    positions of the index range -> (points, unit normals, sorted indices of the planted points)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = np.empty((n, 3))
    p[:, :2] = rng.uniform(-0.4, 0.6, size=(n, 2))
    p[:, 2] = rng.normal(0.0, 0.002, size=n)
    m = -(-n // 50)
    planted = np.sort(rng.choice(n, size=m, replace=False))
    p[planted, 2] = rng.uniform(0.05, 0.30, size=m) * rng.choice([-1.0, 1.0], size=m)
    nr = rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return p, nr, planted


def lattice_cloud():
    """A 12 x 12 x 2 lattice of pitch 0.005 (exact ties at the k-th place) followed by a 5-point cluster 3 m away along x: 293 points."""
    g = np.arange(12) * 0.005
    lat = np.array([[x, y, z] for z in (0.0, 0.005) for y in g for x in g])
    rng = np.random.Generator(np.random.PCG64(5))
    far = np.array([3.0, 0.02, 0.0]) + rng.uniform(-0.004, 0.004, size=(5, 3))
    p = np.vstack([lat, far])
    nr = rng.normal(size=(len(p), 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return p, nr


def tie_count(p, k):
    """Points whose k-th and k+1-th neighbour values (self at place 0) are exactly equal."""
    n = len(p)
    D = np.sort(dist2_matrix(p), axis=1)
    return int((D[:, k] == D[:, min(k + 1, n - 1)]).sum()) if n > k + 1 else 0
