"""The contract of mvicp_fit_normals (include/mvicp.h) in numpy (`fit`), and the same statement as a plain Python loop over scalar floats
(`fit_loop`).  Per point: the normal n, curvature and count of mvicp_estimate_normals (normref), a tangent frame (u, v) from n alone, the
offsets of the row in that frame scaled by the largest offset length, the normal equations of a height polynomial of degree 2 or 3 over
(X, Y) by the pairwise tree sum of 64 leaves, a Cholesky factorisation with a relative pivot threshold, and the normal from the two slope
coefficients.  A point whose fit is refused keeps the estimate's bytes.  Every operation is one fp64 operation of numpy or of a Python
float: rounded on its own, never fused."""
import math

import numpy as np

import normref

LEAVES = normref.LEAVES
PIVOT = 2.0 ** -20    # a pivot s of column j passes iff s > PIVOT * G[j][j]
TERMS = {2: 6, 3: 10}  # the monomials 1, X, Y, X2, XY, Y2 (, X3, X2Y, XY2, Y3)


def check_args(max_nn, radius, viewpoint, degree):
    if degree not in TERMS:
        raise ValueError("degree must be 2 or 3")
    return normref.check_args(max_nn, radius, viewpoint)


def _basis(one, X, Y, degree):
    """the monomial list of the contract from 1, X and Y (arrays or floats), products in the stated order"""
    X2, XY, Y2 = X * X, X * Y, Y * Y
    b = [one, X, Y, X2, XY, Y2]
    if degree == 3:
        b += [X2 * X, X2 * Y, X * Y2, Y2 * Y]
    return b


def fit(p, max_nn=16, radius=0.0, viewpoint=None, degree=3, rows=None):
    """-> dict(nrm (n, 3), curvature (n,), used (n,) int32, fitted (n,) uint8) and, for the tests, knn = the rows."""
    check_args(max_nn, radius, viewpoint, degree)
    M = TERMS[degree]
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    base = normref.normals(p, max_nn, radius, viewpoint, rows)
    rows = base["knn"]
    out = {"nrm": base["nrm"].copy(), "curvature": base["curvature"], "used": base["used"], "fitted": np.zeros(n, dtype=np.uint8), "knn": rows}
    if n == 0:
        return out
    cnt = rows["cnt"].astype(np.int64)
    idx = np.zeros((n, LEAVES), dtype=np.int64)
    idx[:, :max_nn] = np.maximum(rows["idx"], 0)
    inside = np.arange(LEAVES)[None, :] < cnt[:, None]
    with np.errstate(all="ignore"):
        d = np.where(inside[:, :, None], p[idx] - p[:, None, :], 0.0)      # (n, 64, 3)
        N = base["nrm"]
        # the tangent frame: w = e_a x n for the axis a of the smallest |n_a| (the first of equals), u = w / |w|, v = n x u
        a = np.argmin(np.abs(N), axis=1)
        zero = np.zeros(n)
        w = np.where((a == 0)[:, None], np.stack([zero, -N[:, 2], N[:, 1]], 1),
                     np.where((a == 1)[:, None], np.stack([N[:, 2], zero, -N[:, 0]], 1), np.stack([-N[:, 1], N[:, 0], zero], 1)))
        u = w / np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]
        v = np.stack([N[:, 1] * u[:, 2] - N[:, 2] * u[:, 1], N[:, 2] * u[:, 0] - N[:, 0] * u[:, 2], N[:, 0] * u[:, 1] - N[:, 1] * u[:, 0]], 1)
        h = np.sqrt(((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).max(axis=1))
        ok = (cnt >= M) & ~(h == 0)

        def coord(e):
            return np.where(inside, ((d[:, :, 0] * e[:, None, 0] + d[:, :, 1] * e[:, None, 1]) + d[:, :, 2] * e[:, None, 2]) / h[:, None], 0.0)
        X, Y, Z = coord(u), coord(v), coord(N)
        b = [np.where(inside, t, 0.0) for t in _basis(np.ones_like(X), X, Y, degree)]
        G = np.zeros((n, M, M))
        for m in range(M):
            for l in range(m, M):
                G[:, m, l] = G[:, l, m] = normref.tree_sum(b[m] * b[l])
        r = np.stack([normref.tree_sum(b[m] * Z) for m in range(M)], 1)
        L = np.zeros((n, M, M))
        for j in range(M):
            s = G[:, j, j].copy()
            for q in range(j):
                s = s - L[:, j, q] * L[:, j, q]
            ok = ok & (s > PIVOT * G[:, j, j])
            L[:, j, j] = np.sqrt(s)
            for rr in range(j + 1, M):
                s = G[:, rr, j].copy()
                for q in range(j):
                    s = s - L[:, rr, q] * L[:, j, q]
                L[:, rr, j] = s / L[:, j, j]
        y = np.zeros((n, M))
        for j in range(M):
            s = r[:, j].copy()
            for q in range(j):
                s = s - L[:, j, q] * y[:, q]
            y[:, j] = s / L[:, j, j]
        c = np.zeros((n, M))           # the coefficients a_m; a_0 is not computed
        for m in range(M - 1, 0, -1):
            s = y[:, m].copy()
            for q in range(M - 1, m, -1):
                s = s - L[:, q, m] * c[:, q]
            c[:, m] = s / L[:, m, m]
        g = (N - c[:, 1:2] * u) - c[:, 2:3] * v
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = ok & np.isfinite(g).all(axis=1) & np.isfinite(ln) & ~(ln == 0)
        nv = g / ln[:, None]
    out["nrm"] = np.ascontiguousarray(np.where(ok[:, None], nv, base["nrm"]))
    out["fitted"] = ok.astype(np.uint8)
    return out


def fit_loop(p, max_nn=16, radius=0.0, viewpoint=None, degree=3, rows=None):
    """The same contract, one scalar operation at a time on Python floats (step 1 from normref.normals_loop)."""
    check_args(max_nn, radius, viewpoint, degree)
    M = TERMS[degree]
    P = [[float(x) for x in row] for row in np.asarray(p, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    base = normref.normals_loop(np.asarray(P).reshape(-1, 3), max_nn, radius, viewpoint, rows)
    rows = base["knn"]
    nrm, fitted = base["nrm"].copy(), np.zeros(n, dtype=np.uint8)
    for i in range(n):
        c = int(rows["cnt"][i])
        if c < M:
            continue
        N = [float(x) for x in base["nrm"][i]]
        d = [[P[int(rows["idx"][i][t])][k] - P[i][k] for k in range(3)] for t in range(c)]
        a = 0
        if abs(N[1]) < abs(N[a]):
            a = 1
        if abs(N[2]) < abs(N[a]):
            a = 2
        w = [[0.0, -N[2], N[1]], [N[2], 0.0, -N[0]], [-N[1], N[0], 0.0]][a]
        lw = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        u = [w[k] / lw for k in range(3)]
        v = [N[1] * u[2] - N[2] * u[1], N[2] * u[0] - N[0] * u[2], N[0] * u[1] - N[1] * u[0]]
        h2 = 0.0
        for t in range(c):
            h2 = max(h2, (d[t][0] * d[t][0] + d[t][1] * d[t][1]) + d[t][2] * d[t][2])
        h = math.sqrt(h2)
        if h == 0:
            continue
        b = [[0.0] * LEAVES for _ in range(M)]
        Z = [0.0] * LEAVES
        for t in range(c):
            X, Y, Z[t] = (((d[t][0] * e[0] + d[t][1] * e[1]) + d[t][2] * e[2]) / h for e in (u, v, N))
            for m, val in enumerate(_basis(1.0, X, Y, degree)):
                b[m][t] = val
        tsum = normref._tree_sum_scalar
        G = [[0.0] * M for _ in range(M)]
        for m in range(M):
            for l in range(m, M):
                G[m][l] = G[l][m] = tsum([b[m][t] * b[l][t] for t in range(LEAVES)])
        r = [tsum([b[m][t] * Z[t] for t in range(LEAVES)]) for m in range(M)]
        L = [[0.0] * M for _ in range(M)]
        ok = True
        for j in range(M):
            s = G[j][j]
            for q in range(j):
                s = s - L[j][q] * L[j][q]
            if not s > PIVOT * G[j][j]:
                ok = False
                break
            L[j][j] = math.sqrt(s)
            for rr in range(j + 1, M):
                s = G[rr][j]
                for q in range(j):
                    s = s - L[rr][q] * L[j][q]
                L[rr][j] = s / L[j][j]
        if not ok:
            continue
        y = [0.0] * M
        for j in range(M):
            s = r[j]
            for q in range(j):
                s = s - L[j][q] * y[q]
            y[j] = s / L[j][j]
        co = [0.0] * M
        for m in range(M - 1, 0, -1):
            s = y[m]
            for q in range(M - 1, m, -1):
                s = s - L[q][m] * co[q]
            co[m] = s / L[m][m]
        g = [(N[k] - co[1] * u[k]) - co[2] * v[k] for k in range(3)]
        if not all(math.isfinite(x) for x in g):
            continue
        ln = math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
        if not math.isfinite(ln) or ln == 0:
            continue
        nrm[i] = [g[k] / ln for k in range(3)]
        fitted[i] = 1
    return {"nrm": nrm, "curvature": base["curvature"], "used": base["used"], "fitted": fitted, "knn": rows}


KEYS = normref.KEYS + (("fitted", np.uint8),)


def same(a, b):
    """Byte equality of two results (signs of zeros included)."""
    for key, dt in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def angle_deg(a, b):
    """the angle between the rows of a and b up to sign, in degrees"""
    c = np.abs((a * b).sum(1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    s = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arctan2(s, c))
