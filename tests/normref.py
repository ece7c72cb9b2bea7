"""The contract of mvicp_estimate_normals (include/mvicp.h) in numpy (`normals`), and the same statement as a plain Python loop over
scalar floats (`normals_loop`).  Per point: the offsets from the point to the entries of its self-mode mvicp_knn_search row (knnref), their
mean and second moments by a pairwise tree sum of 64 leaves, the Jacobi iteration of the ISS contract with the vectors, the vector of the
smallest diagonal entry normalised and turned towards the viewpoint, and the surface variation.  Every operation is one fp64 operation of
numpy or of a Python float: rounded on its own, never fused."""
import math

import numpy as np

import knnref

LEAVES = 64
SWEEPS = 6
PAIRS = ((0, 1), (0, 2), (1, 2))


def check_args(max_nn, radius, viewpoint):
    if not 3 <= max_nn <= LEAVES:
        raise ValueError("needs 3 <= max_nn <= 64")
    if not math.isfinite(radius):
        raise ValueError("radius must be finite (<= 0: no radius)")
    vp = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, dtype=np.float64).reshape(3)
    if not np.isfinite(vp).all():
        raise ValueError("viewpoint must be finite")
    return vp


def tree_sum(y):
    """T(y) over the last axis (64 long): six times y[u] <- y[2u] + y[2u+1]"""
    assert y.shape[-1] == LEAVES
    while y.shape[-1] > 1:
        y = y[..., 0::2] + y[..., 1::2]
    return y[..., 0]


def _jacobi(A, V):
    """SWEEPS sweeps over PAIRS on the (n, 3, 3) stacks A and V, in place; a rotation is skipped iff A[p][q] == 0"""
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                on = A[:, p, q] != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * A[:, p, q])
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                B, W = A.copy(), V.copy()
                for r in range(3):
                    arp, arq = B[:, r, p].copy(), B[:, r, q].copy()
                    B[:, r, p] = c * arp - s * arq; B[:, r, q] = s * arp + c * arq
                for r in range(3):
                    apr, aqr = B[:, p, r].copy(), B[:, q, r].copy()
                    B[:, p, r] = c * apr - s * aqr; B[:, q, r] = s * apr + c * aqr
                for r in range(3):
                    vrp, vrq = W[:, r, p].copy(), W[:, r, q].copy()
                    W[:, r, p] = c * vrp - s * vrq; W[:, r, q] = s * vrp + c * vrq
                A[on] = B[on]; V[on] = W[on]
    return A, V


def normals(p, max_nn=30, radius=0.0, viewpoint=None, rows=None):
    """-> dict(nrm (n, 3), curvature (n,), used (n,) int32) and, for the tests, knn = the rows (knnref.knn_search(p, None, max_nn, radius),
    or `rows` if the caller has them already)."""
    vp = check_args(max_nn, radius, viewpoint)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if rows is None:
        rows = knnref.knn_search(p, None, max_nn, radius)
    cnt = rows["cnt"].astype(np.int64)
    nrm, curv = np.zeros((n, 3)), np.zeros(n)
    if n:
        idx = np.full((n, LEAVES), -1, dtype=np.int64)
        idx[:, :max_nn] = rows["idx"]
        inside = np.arange(LEAVES)[None, :] < cnt[:, None]
        assert ((idx >= 0) == inside).all()
        ok = cnt >= 3
        with np.errstate(all="ignore"):
            d = np.where(inside[:, :, None], p[np.where(inside, idx, 0)] - p[:, None, :], 0.0)      # (n, 64, 3)
            mean = tree_sum(np.moveaxis(d, 1, 2)) / np.maximum(cnt, 1).astype(np.float64)[:, None]  # (n, 3)
            x = np.where(inside[:, :, None], d - mean[:, None, :], 0.0)
            A = np.zeros((n, 3, 3))
            for a in range(3):
                for b in range(a, 3):
                    A[:, a, b] = A[:, b, a] = tree_sum(x[:, :, a] * x[:, :, b])
            V = np.zeros((n, 3, 3)); V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1.0
            A, V = _jacobi(A, V)
            ar = np.arange(n)
            m = np.zeros(n, dtype=np.int64)
            m = np.where(A[:, 1, 1] < A[ar, m, m], 1, m)
            m = np.where(A[:, 2, 2] < A[ar, m, m], 2, m)
            v = V[ar, :, m]
            ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            nv = v / ln[:, None]
            w = vp[None, :] - p
            s = (nv[:, 0] * w[:, 0] + nv[:, 1] * w[:, 1]) + nv[:, 2] * w[:, 2]
            nv = np.where((s < 0)[:, None], -nv, nv)
            S = (A[:, 0, 0] + A[:, 1, 1]) + A[:, 2, 2]
            l = A[ar, m, m]
            cv = np.where((l > 0) & (S > 0), l / S, 0.0)
        nrm = np.where(ok[:, None], nv, 0.0)
        curv = np.where(ok, cv, 0.0)
    return {"nrm": np.ascontiguousarray(nrm), "curvature": np.ascontiguousarray(curv), "used": cnt.astype(np.int32), "knn": rows}


def _tree_sum_scalar(y):
    y = list(y)
    assert len(y) == LEAVES
    while len(y) > 1:
        y = [y[2 * u] + y[2 * u + 1] for u in range(len(y) // 2)]
    return y[0]


def normals_loop(p, max_nn=30, radius=0.0, viewpoint=None, rows=None):
    """The same contract, one scalar operation at a time on Python floats (rows: from knnref.knn_search_loop unless given)."""
    vp = [float(v) for v in check_args(max_nn, radius, viewpoint)]
    P = [[float(v) for v in row] for row in np.asarray(p, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    if rows is None:
        rows = knnref.knn_search_loop(np.asarray(P).reshape(-1, 3), None, max_nn, radius)
    nrm, curv, used = np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.int32)
    for i in range(n):
        c = int(rows["cnt"][i])
        used[i] = c
        if c < 3:
            continue
        d = [[0.0, 0.0, 0.0] for _ in range(LEAVES)]
        for t in range(c):
            j = int(rows["idx"][i][t])
            d[t] = [P[j][a] - P[i][a] for a in range(3)]
        mean = [_tree_sum_scalar([d[t][a] for t in range(LEAVES)]) / float(c) for a in range(3)]
        x = [[d[t][a] - mean[a] for a in range(3)] if t < c else [0.0, 0.0, 0.0] for t in range(LEAVES)]
        A = [[0.0] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(a, 3):
                A[a][b] = A[b][a] = _tree_sum_scalar([x[t][a] * x[t][b] for t in range(LEAVES)])
        V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
        for _ in range(SWEEPS):
            for pp, q in PAIRS:
                if A[pp][q] == 0:
                    continue
                theta = (A[q][q] - A[pp][pp]) / (2.0 * A[pp][q])
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                cc = 1.0 / math.sqrt(t * t + 1.0)
                s = t * cc
                for r in range(3):
                    arp, arq = A[r][pp], A[r][q]
                    A[r][pp] = cc * arp - s * arq; A[r][q] = s * arp + cc * arq
                for r in range(3):
                    apr, aqr = A[pp][r], A[q][r]
                    A[pp][r] = cc * apr - s * aqr; A[q][r] = s * apr + cc * aqr
                for r in range(3):
                    vrp, vrq = V[r][pp], V[r][q]
                    V[r][pp] = cc * vrp - s * vrq; V[r][q] = s * vrp + cc * vrq
        m = 0
        if A[1][1] < A[m][m]:
            m = 1
        if A[2][2] < A[m][m]:
            m = 2
        v = [V[0][m], V[1][m], V[2][m]]
        ln = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nv = [v[a] / ln for a in range(3)]
        w = [vp[a] - P[i][a] for a in range(3)]
        s = (nv[0] * w[0] + nv[1] * w[1]) + nv[2] * w[2]
        if s < 0:
            nv = [-nv[a] for a in range(3)]
        S = (A[0][0] + A[1][1]) + A[2][2]
        l = A[m][m]
        nrm[i] = nv
        curv[i] = l / S if l > 0 and S > 0 else 0.0
    return {"nrm": nrm, "curvature": curv, "used": used, "knn": rows}


KEYS = (("nrm", np.float64), ("curvature", np.float64), ("used", np.int32))


def same(a, b):
    """Byte equality of two results (signs of zeros included)."""
    for key, dt in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True
