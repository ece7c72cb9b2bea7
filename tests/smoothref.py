"""The contract of mvicp_smooth_points (include/mvicp.h) in numpy (`smooth`), and the same statement as a plain Python loop over scalar
floats (`smooth_loop`).  Per point: the fit of mvicp_fit_normals (jetref) with the back substitution continued to a_0, the height of the
fitted polynomial at the point; the point moved by a_0 * h along its PCA normal (normref); the mean and the Gaussian curvature of the
polynomial.  nrm, curvature, used and fitted are jetref's bytes.  Every operation is one fp64 operation of numpy or of a Python float:
rounded on its own, never fused."""
import math

import numpy as np

import jetref
import normref

LEAVES = normref.LEAVES
TERMS = jetref.TERMS


def check_args(max_nn, radius, viewpoint, degree, max_shift):
    if math.isnan(float(max_shift)):
        raise ValueError("max_shift must not be a NaN")
    return jetref.check_args(max_nn, radius, viewpoint, degree)


def smooth(p, max_nn=30, radius=0.0, viewpoint=None, degree=2, max_shift=0.0, rows=None):
    """-> dict(xyz (n, 3), shift (n,), moved (n,) uint8, H (n,), K (n,), and jetref.fit's nrm, curvature, used, fitted, knn)."""
    check_args(max_nn, radius, viewpoint, degree, max_shift)
    M = TERMS[degree]
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    out = dict(jetref.fit(p, max_nn, radius, viewpoint, degree, rows))
    rows = out["knn"]
    out.update(xyz=p.copy(), shift=np.zeros(n), moved=np.zeros(n, dtype=np.uint8), H=np.zeros(n), K=np.zeros(n))
    if n == 0:
        return out
    N = normref.normals(p, max_nn, radius, viewpoint, rows)["nrm"]      # the PCA normal of step 1
    fitted = out["fitted"].astype(bool)
    cnt = rows["cnt"].astype(np.int64)
    idx = np.zeros((n, LEAVES), dtype=np.int64)
    idx[:, :max_nn] = np.maximum(rows["idx"], 0)
    inside = np.arange(LEAVES)[None, :] < cnt[:, None]
    with np.errstate(all="ignore"):
        # steps 4 to 9 as jetref.fit states them
        d = np.where(inside[:, :, None], p[idx] - p[:, None, :], 0.0)
        a = np.argmin(np.abs(N), axis=1)
        zero = np.zeros(n)
        w = np.where((a == 0)[:, None], np.stack([zero, -N[:, 2], N[:, 1]], 1),
                     np.where((a == 1)[:, None], np.stack([N[:, 2], zero, -N[:, 0]], 1), np.stack([-N[:, 1], N[:, 0], zero], 1)))
        u = w / np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]
        v = np.stack([N[:, 1] * u[:, 2] - N[:, 2] * u[:, 1], N[:, 2] * u[:, 0] - N[:, 0] * u[:, 2], N[:, 0] * u[:, 1] - N[:, 1] * u[:, 0]], 1)
        h = np.sqrt(((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]).max(axis=1))

        def coord(e):
            return np.where(inside, ((d[:, :, 0] * e[:, None, 0] + d[:, :, 1] * e[:, None, 1]) + d[:, :, 2] * e[:, None, 2]) / h[:, None], 0.0)
        X, Y, Z = coord(u), coord(v), coord(N)
        b = [np.where(inside, t, 0.0) for t in jetref._basis(np.ones_like(X), X, Y, degree)]
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
        c = np.zeros((n, M))
        for m in range(M - 1, -1, -1):           # step 9a: down to a_0
            s = y[:, m].copy()
            for q in range(M - 1, m, -1):
                s = s - L[:, q, m] * c[:, q]
            c[:, m] = s / L[:, m, m]
        # 11 shift, 12 projection
        ah = c[:, 0] * h
        fin = fitted & np.isfinite(ah)
        shift = np.where(fin, ah, 0.0)
        x = p + shift[:, None] * N
        moved = fin & np.isfinite(x).all(axis=1)
        if max_shift > 0:
            moved = moved & (np.abs(shift) <= max_shift)
        # 13 curvatures
        a1, a2, a3, a4, a5 = (c[:, m] for m in range(1, 6))
        E, Gm, F = 1.0 + a1 * a1, 1.0 + a2 * a2, a1 * a2
        w2 = E + a2 * a2
        ww = np.sqrt(w2)
        zxx, zxy, zyy = (a3 + a3) / h, a4 / h, (a5 + a5) / h
        Hm = ((Gm * zxx - (F + F) * zxy) + E * zyy) / ((w2 * ww) + (w2 * ww))
        Kg = (zxx * zyy - zxy * zxy) / (w2 * w2)
        good = fitted & np.isfinite(Hm) & np.isfinite(Kg)
    out["shift"] = np.ascontiguousarray(shift)
    out["xyz"] = np.ascontiguousarray(np.where(moved[:, None], x, p))
    out["moved"] = moved.astype(np.uint8)
    out["H"] = np.ascontiguousarray(np.where(good, Hm, 0.0))
    out["K"] = np.ascontiguousarray(np.where(good, Kg, 0.0))
    return out


def smooth_loop(p, max_nn=30, radius=0.0, viewpoint=None, degree=2, max_shift=0.0, rows=None):
    """The same contract, one scalar operation at a time on Python floats (steps 1 to 10 from jetref.fit_loop; a row it did not fit is
    not touched again)."""
    check_args(max_nn, radius, viewpoint, degree, max_shift)
    M = TERMS[degree]
    P = [[float(x) for x in row] for row in np.asarray(p, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    arr = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    out = dict(jetref.fit_loop(arr, max_nn, radius, viewpoint, degree, rows))
    rows = out["knn"]
    base = normref.normals_loop(arr, max_nn, radius, viewpoint, rows)["nrm"]
    xyz, shift, moved, Hs, Ks = arr.copy(), np.zeros(n), np.zeros(n, dtype=np.uint8), np.zeros(n), np.zeros(n)
    tsum = normref._tree_sum_scalar
    for i in range(n):
        if not out["fitted"][i]:
            continue
        cn = int(rows["cnt"][i])
        N = [float(x) for x in base[i]]
        d = [[P[int(rows["idx"][i][t])][k] - P[i][k] for k in range(3)] for t in range(cn)]
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
        for t in range(cn):
            h2 = max(h2, (d[t][0] * d[t][0] + d[t][1] * d[t][1]) + d[t][2] * d[t][2])
        h = math.sqrt(h2)
        b = [[0.0] * LEAVES for _ in range(M)]
        Z = [0.0] * LEAVES
        for t in range(cn):
            X, Y, Z[t] = (((d[t][0] * e[0] + d[t][1] * e[1]) + d[t][2] * e[2]) / h for e in (u, v, N))
            for m, val in enumerate(jetref._basis(1.0, X, Y, degree)):
                b[m][t] = val
        G = [[0.0] * M for _ in range(M)]
        for m in range(M):
            for l in range(m, M):
                G[m][l] = G[l][m] = tsum([b[m][t] * b[l][t] for t in range(LEAVES)])
        r = [tsum([b[m][t] * Z[t] for t in range(LEAVES)]) for m in range(M)]
        L = [[0.0] * M for _ in range(M)]
        for j in range(M):
            s = G[j][j]
            for q in range(j):
                s = s - L[j][q] * L[j][q]
            L[j][j] = math.sqrt(s)
            for rr in range(j + 1, M):
                s = G[rr][j]
                for q in range(j):
                    s = s - L[rr][q] * L[j][q]
                L[rr][j] = s / L[j][j]
        y = [0.0] * M
        for j in range(M):
            s = r[j]
            for q in range(j):
                s = s - L[j][q] * y[q]
            y[j] = s / L[j][j]
        co = [0.0] * M
        for m in range(M - 1, -1, -1):
            s = y[m]
            for q in range(M - 1, m, -1):
                s = s - L[q][m] * co[q]
            co[m] = s / L[m][m]
        ah = co[0] * h
        if math.isfinite(ah):
            shift[i] = ah
            x = [P[i][k] + ah * N[k] for k in range(3)]
            if all(math.isfinite(t) for t in x) and (max_shift <= 0 or abs(ah) <= max_shift):
                xyz[i] = x
                moved[i] = 1
        E, Gm, F = 1.0 + co[1] * co[1], 1.0 + co[2] * co[2], co[1] * co[2]
        w2 = E + co[2] * co[2]
        ww = math.sqrt(w2)
        zxx, zxy, zyy = (co[3] + co[3]) / h, co[4] / h, (co[5] + co[5]) / h
        den_h, den_k = (w2 * ww) + (w2 * ww), w2 * w2
        num_h, num_k = (Gm * zxx - (F + F) * zxy) + E * zyy, zxx * zyy - zxy * zxy
        if den_h != 0 and den_k != 0:            # (a Python float division by zero raises; w2 >= 1 unless it is a NaN)
            Hm, Kg = num_h / den_h, num_k / den_k
            if math.isfinite(Hm) and math.isfinite(Kg):
                Hs[i], Ks[i] = Hm, Kg
    out.update(xyz=xyz, shift=shift, moved=moved, H=Hs, K=Ks)
    return out


KEYS = jetref.KEYS + (("xyz", np.float64), ("shift", np.float64), ("moved", np.uint8), ("H", np.float64), ("K", np.float64))


def same(a, b, keys=KEYS):
    """Byte equality of two results (signs of zeros included)."""
    for key, dt in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def noisy(p, nrm, sigma, rng):
    """p moved along nrm by Gaussian noise of standard deviation sigma, one draw per point from rng"""
    return np.ascontiguousarray(p + (sigma * rng.standard_normal(len(p)))[:, None] * nrm)
