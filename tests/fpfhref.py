"""The contract of mvicp_fpfh (include/mvicp.h) in numpy, and the same statement as a plain Python loop over scalars (`fpfh_loop`).

FPFH (Rusu 2009; PCL's computePairFeatures / SPFH / weighting, Open3D's ComputeFPFHFeature) restated with + - x / sqrt, comparisons and
floor only, in fp64, every operation rounded on its own (numpy never contracts to fma), in a stated order.  The textbook uses atan2 and
acos, which no library rounds correctly; here the theta bin is the number of the ten inner bin edges the direction (x, y) has passed,
decided by the sign of a cross product with a table of the edges' directions, and the acos|.| comparison of the swap test is the
comparison of the absolute values themselves (acos is strictly decreasing on [0, 1]).  tests/test_fpfh_cpu.py checks against a textbook
evaluation in extended precision that this is the same definition up to rounding at a bin edge.

  N(i)   row i of knnref.knn_search(p, None, max_nn, radius) without its entries with d2 == 0, in row order
  pair   d = p_j - p_i, dist = sqrt(d2) (the row's d2); dot (x0 y0 + x1 y1) + x2 y2; cross x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0
         a1 = n_i . d, a2 = n_j . d; swap iff |a1| < |a2|: (s, t, e, f3) = (n_j, n_i, -d, (-a2) / dist), else (n_i, n_j, d, a1 / dist)
         v = e x s, vn = sqrt(v . v); vn == 0: bins (5, 5, 5); else v = v / vn, w = s x v, f2 = v . t, y = w . t, x = s . t
  bins   f2, f3: min(10, max(0, floor((f + 1.0) * 5.5))); theta: edges k = 1 .. 10 at phi_k = -pi + 2 pi k / 11 with the table EDGES of
         the doubles nearest to (cos phi_k, sin phi_k), cr_k = c_k * y - s_k * x; k <= 5 passed iff y >= 0 or cr_k >= 0; k >= 6 passed
         iff (y > 0 and cr_k >= 0) or (y == 0 and x < 0); the bin is the number of edges passed
  SPFH   integer counts c_i[33] (theta 0-10, f2 11-21, f3 22-32) over N(i), m_i = |N(i)|, r_i = 100.0 / m_i (0 if m_i == 0)
  FPFH   acc = +0.0; over N(i) in row order: g = r_j / d2, acc[b] = acc[b] + c_j[b] * g; per sub-histogram S = sequential sum of its 11
         acc, scale = 100.0 / S if S != 0 else 0; out[i][b] = acc[b] * scale + c_i[b] * r_i
"""
import math

import numpy as np

import knnref

BINS = 33
# (c_k, s_k), k = 1 .. 10: the doubles nearest to cos / sin of -pi + 2 pi k / 11; the same literals as csrc/fpfh.hip
EDGES = tuple((float.fromhex(c), float.fromhex(s)) for c, s in (
    ("-0x1.aeb8c8764f0bap-1", "-0x1.14cedf8bb580bp-1"), ("-0x1.a9628d9c712b6p-2", "-0x1.d1bb48eee2c13p-1"),
    ("0x1.2375f640f44dbp-3", "-0x1.fac9e043842efp-1"), ("0x1.4f49e7f775887p-1", "-0x1.82f19bb3a28a1p-1"),
    ("0x1.eb42a9bcd5057p-1", "-0x1.207e7fd768dbfp-2"), ("0x1.eb42a9bcd5057p-1", "0x1.207e7fd768dbfp-2"),
    ("0x1.4f49e7f775887p-1", "0x1.82f19bb3a28a1p-1"), ("0x1.2375f640f44dbp-3", "0x1.fac9e043842efp-1"),
    ("-0x1.a9628d9c712b6p-2", "0x1.d1bb48eee2c13p-1"), ("-0x1.aeb8c8764f0bap-1", "0x1.14cedf8bb580bp-1")))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _bin11(f):
    return np.minimum(10.0, np.maximum(0.0, np.floor((f + 1.0) * 5.5))).astype(np.int64)


def _theta_bin(x, y):
    b = np.zeros(x.shape, dtype=np.int64)
    for k, (c, s) in enumerate(EDGES):
        cr = c * y - s * x
        b += ((y >= 0) | (cr >= 0)) if k < 5 else (((y > 0) & (cr >= 0)) | ((y == 0) & (x < 0)))
    return b


def pair_bins(p, nrm, knn):
    """-> (valid (n, k) bool, bins (n, k, 3) of the valid pairs, what (n, k, 3) bool: degenerate / y == 0 / swap tie) over the rows of `knn`."""
    n, k = knn["idx"].shape
    valid = (np.arange(k)[None, :] < knn["cnt"][:, None]) & (knn["d2"] != 0)
    j = np.where(valid, knn["idx"], 0)
    d = p[j] - p[:, None, :]
    ni, nj = np.broadcast_to(nrm[:, None, :], (n, k, 3)), nrm[j]
    with np.errstate(all="ignore"):
        dist = np.sqrt(np.where(valid, knn["d2"], 1.0))
        a1, a2 = _dot(ni, d), _dot(nj, d)
        swap = np.abs(a1) < np.abs(a2)
        sw = swap[..., None]
        s, t, e = np.where(sw, nj, ni), np.where(sw, ni, nj), np.where(sw, -d, d)
        f3 = np.where(swap, -a2, a1) / dist
        v = _cross(e, s)
        vn = np.sqrt(_dot(v, v))
        deg = vn == 0
        v = v / np.where(deg, 1.0, vn)[..., None]
        w = _cross(s, v)
        f2, y, x = _dot(v, t), _dot(w, t), _dot(s, t)
        bins = np.stack([_theta_bin(x, y), _bin11(f2), _bin11(f3)], -1)
    bins[deg] = 5
    what = np.stack([deg, ~deg & (y == 0), np.abs(a1) == np.abs(a2)], -1) & valid[..., None]
    return valid, bins, what


def fpfh(p, nrm, radius, max_nn=64, knn=None):
    """-> dict(desc (n, 33) float64, used (n,) int32 = m_i, spfh (n, 33) uint8, r (n,), valid, bins, and the counts over all pairs
    `degenerate` / `y_zero` / `swap_ties` / `pairs`).  knn: the rows knnref.knn_search(p, None, max_nn, radius), if the caller has them."""
    if not (2 <= max_nn <= 64 and radius > 0 and math.isfinite(radius)):
        raise ValueError("needs 2 <= max_nn <= 64 and a finite radius > 0")
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    nrm = np.ascontiguousarray(nrm, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if knn is None:
        knn = knnref.knn_search(p, None, max_nn, radius)
    valid, bins, what = pair_bins(p, nrm, knn)
    rows = np.broadcast_to(np.arange(n)[:, None], valid.shape)[valid]
    c = np.zeros((n, BINS), dtype=np.int64)
    for f in range(3):
        c += np.bincount(rows * BINS + 11 * f + bins[..., f][valid], minlength=n * BINS).reshape(n, BINS)
    m = valid.sum(1)
    with np.errstate(all="ignore"):
        r = np.where(m > 0, 100.0 / np.maximum(m, 1).astype(np.float64), 0.0)
        cf = c.astype(np.float64)
        acc = np.zeros((n, BINS))
        for t in range(valid.shape[1]):
            on = valid[:, t]
            jt = np.where(on, knn["idx"][:, t], 0)
            g = r[jt] / np.where(on, knn["d2"][:, t], 1.0)
            acc = np.where(on[:, None], acc + cf[jt] * g[:, None], acc)
        desc = np.zeros((n, BINS))
        for f in range(3):
            S = np.zeros(n)
            for b in range(11 * f, 11 * f + 11):
                S = S + acc[:, b]
            scale = np.where(S != 0, 100.0 / np.where(S != 0, S, 1.0), 0.0)
            desc[:, 11 * f:11 * f + 11] = acc[:, 11 * f:11 * f + 11] * scale[:, None] + cf[:, 11 * f:11 * f + 11] * r[:, None]
    return {"desc": desc, "used": m.astype(np.int32), "spfh": c.astype(np.uint8), "r": r, "valid": valid, "bins": bins,
            "degenerate": int(what[..., 0].sum()), "y_zero": int(what[..., 1].sum()), "swap_ties": int(what[..., 2].sum()), "pairs": int(valid.sum())}


def fpfh_loop(p, nrm, radius, max_nn=64):
    """The same contract, one scalar operation at a time -> dict(desc, used, spfh)."""
    n = len(p)
    P = [[float(x) for x in row] for row in p]
    Nr = [[float(x) for x in row] for row in nrm]
    knn = knnref.knn_search_loop(p, None, max_nn, radius)

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def bin11(f):
        return int(min(10.0, max(0.0, math.floor((f + 1.0) * 5.5))))

    rows = [[(int(knn["idx"][i, t]), float(knn["d2"][i, t])) for t in range(int(knn["cnt"][i])) if knn["d2"][i, t] != 0] for i in range(n)]
    c = [[0] * BINS for _ in range(n)]
    for i in range(n):
        for j, d2 in rows[i]:
            d = [P[j][0] - P[i][0], P[j][1] - P[i][1], P[j][2] - P[i][2]]
            dist = math.sqrt(d2)
            a1, a2 = dot(Nr[i], d), dot(Nr[j], d)
            if abs(a1) < abs(a2):
                s, t, e, f3 = Nr[j], Nr[i], [-d[0], -d[1], -d[2]], (-a2) / dist
            else:
                s, t, e, f3 = Nr[i], Nr[j], d, a1 / dist
            v = cross(e, s)
            vn = math.sqrt(dot(v, v))
            if vn == 0:
                b0 = b1 = b2 = 5
            else:
                v = [v[0] / vn, v[1] / vn, v[2] / vn]
                w = cross(s, v)
                f2, y, x = dot(v, t), dot(w, t), dot(s, t)
                b0 = 0
                for k, (ck, sk) in enumerate(EDGES):
                    cr = ck * y - sk * x
                    if k < 5:
                        b0 += 1 if (y >= 0 or cr >= 0) else 0
                    else:
                        b0 += 1 if ((y > 0 and cr >= 0) or (y == 0 and x < 0)) else 0
                b1, b2 = bin11(f2), bin11(f3)
            c[i][b0] += 1; c[i][11 + b1] += 1; c[i][22 + b2] += 1
    m = [len(row) for row in rows]
    r = [100.0 / float(mi) if mi else 0.0 for mi in m]
    desc = np.zeros((n, BINS))
    for i in range(n):
        acc = [0.0] * BINS
        for j, d2 in rows[i]:
            g = r[j] / d2
            for b in range(BINS):
                acc[b] = acc[b] + float(c[j][b]) * g
        for f in range(3):
            S = 0.0
            for b in range(11 * f, 11 * f + 11):
                S = S + acc[b]
            scale = 100.0 / S if S != 0 else 0.0
            for b in range(11 * f, 11 * f + 11):
                desc[i, b] = acc[b] * scale + float(c[i][b]) * r[i]
    return {"desc": desc, "used": np.array(m, dtype=np.int32), "spfh": np.array(c, dtype=np.uint8).reshape(n, BINS)}


def same(a, b, keys=("desc", "used", "spfh")):
    """Byte equality of two results."""
    for key in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


# ---- the clouds of the tests
def unit_normals(n, seed):
    v = np.random.Generator(np.random.PCG64(seed)).normal(size=(n, 3))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True))


def z_normals(n):
    return np.ascontiguousarray(np.tile([[0.0, 0.0, 1.0]], (n, 1)))
