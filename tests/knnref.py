"""The contract of mvicp_knn_search (include/mvicp.h) in numpy: the brute-force m x n distance matrix in the metric's operation order, a
stable argsort per row -- which IS the order (dist2 ascending, original index ascending) -- and the radius predicate sqrt(D) < radius.
`knn_search_loop` is the same statement as a plain Python loop over scalars."""
import math

import numpy as np


def dist2_matrix(q, p):
    """(d0 d0 + d1 d1) + d2 d2 with d = q - p for all pairs, every operation rounded on its own (numpy never contracts to fma)."""
    d = q[:, None, :] - p[None, :, :]
    return (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]


def sorted_rows(p, q=None):
    """(order (m, n) int32, Ds (m, n)): per query every point of the cloud in the contract's order and its dist2.  A stable argsort of the
    row by dist2 keeps equal values in ascending index."""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    q = p if q is None else np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 3)
    m, n = len(q), len(p)
    order, Ds = np.zeros((m, n), dtype=np.int32), np.zeros((m, n))
    for a in range(0, m, 256):   # slabs: no m x n x 3 temporary for the whole query set
        D = dist2_matrix(q[a:a + 256], p)
        o = np.argsort(D, axis=1, kind="stable")
        order[a:a + 256] = o
        Ds[a:a + 256] = np.take_along_axis(D, o, axis=1)
    return order, Ds


def from_sorted(order, Ds, k, radius):
    """The result for (k, radius) from sorted_rows: the candidates are a prefix of the sorted row (sqrt is monotone)."""
    if not 0 <= k <= 64 or (k == 0 and not radius > 0):
        raise ValueError("needs 0 <= k <= 64, and radius > 0 with k == 0")
    m, n = Ds.shape
    if radius > 0:
        cand = np.sqrt(Ds) < radius
        c = cand.sum(1)
        assert (cand == (np.arange(n)[None, :] < c[:, None])).all()
    else:
        c = np.full(m, n)
    if k:
        c = np.minimum(c, k)
    cnt = c.astype(np.int32)
    total = int(cnt.sum())
    if k:
        w = min(k, n)
        idx, d2 = np.full((m, k), -1, dtype=np.int32), np.full((m, k), np.inf)
        take = np.arange(w)[None, :] < c[:, None]
        idx[:, :w][take] = order[:, :w][take]; d2[:, :w][take] = Ds[:, :w][take]
        off = np.arange(m + 1, dtype=np.int64) * k
    else:
        take = np.arange(n)[None, :] < c[:, None]
        idx, d2 = np.ascontiguousarray(order[take], dtype=np.int32), np.ascontiguousarray(Ds[take])   # (row-major: row after row)
        off = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    return {"cnt": cnt, "off": off, "idx": idx, "d2": d2, "total": total}


def knn_search(p, q=None, k=8, radius=0.0):
    """-> dict(cnt (m,) int32, off (m+1,) int64, idx, d2, total): k >= 1: idx / d2 are (m, k), padded with -1 / +inf, off[i] = i k;
    k == 0 (needs radius > 0): idx / d2 are flat CSR arrays with off[m] entries.  q None: the cloud's own points (self mode)."""
    return from_sorted(*sorted_rows(p, q), k, radius)


def knn_search_loop(p, q=None, k=8, radius=0.0):
    """The same contract, one scalar operation at a time."""
    q = p if q is None else q
    cnt, rows = [], []
    for i in range(len(q)):
        cands = []
        for j in range(len(p)):
            d0, d1, d2 = float(q[i][0]) - float(p[j][0]), float(q[i][1]) - float(p[j][1]), float(q[i][2]) - float(p[j][2])
            d = (d0 * d0 + d1 * d1) + d2 * d2
            if not radius > 0 or math.sqrt(d) < radius:
                cands.append((d, j))
        cands.sort()   # tuples: by d, then by j
        if k:
            cands = cands[:k]
        cnt.append(len(cands)); rows.append(cands)
    m = len(rows)
    if k:
        idx, dd = np.full((m, k), -1, dtype=np.int32), np.full((m, k), np.inf)
        for i, row in enumerate(rows):
            for t, (d, j) in enumerate(row):
                idx[i, t] = j; dd[i, t] = d
        off = np.array([i * k for i in range(m + 1)], dtype=np.int64)
    else:
        idx = np.array([j for row in rows for d, j in row], dtype=np.int32)
        dd = np.array([d for row in rows for d, j in row], dtype=np.float64)
        off = np.zeros(m + 1, dtype=np.int64)
        for i in range(m):
            off[i + 1] = off[i] + cnt[i]
    return {"cnt": np.array(cnt, dtype=np.int32), "off": off, "idx": idx, "d2": dd, "total": int(sum(cnt))}


KEYS = (("cnt", np.int32), ("off", np.int64), ("idx", np.int32), ("d2", np.float64))


def same(a, b):
    """Byte equality of two results."""
    for key, dt in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return int(a["total"]) == int(b["total"])


# ---- the clouds of the tests
def shuffled_lattice(side=7, seed=3):
    """The side^3 integer lattice in a shuffled index order: index order is unrelated to space, distances tie exactly."""
    g = np.arange(side, dtype=np.float64)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.ascontiguousarray(lat[rng.permutation(len(lat))])
