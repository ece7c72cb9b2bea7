"""The contracts of mvicp_feature_match, mvicp_match_pairs and mvicp_consensus (include/mvicp.h) in numpy, and the same statements as
plain Python loops over scalars (`*_loop`).  fp64 throughout, every operation rounded on its own (numpy never contracts to fma); only
+ - x / sqrt and comparisons occur; comparisons are IEEE as written.

  dist(a, b)   s = +0.0; for c = 0 .. dim-1 ascending: t = a[c] - b[c]; s = s + t * t            (symmetric bit for bit)
  match        forward: per row i of A the rows of B ordered by (dist, j), the first two -> fwd_idx / fwd_d2 (m, 2), a missing entry
               padded with (-1, +inf); backward the same per row j of B over the rows of A -> bwd_idx / bwd_d2 (n, 2)
  pairs        (i, j = fwd_idx[i][0]) kept iff j >= 0, (not mutual or bwd_idx[j][0] == i) and
               (ratio >= 1 or fwd_d2[i][0] <= (ratio * ratio) * fwd_d2[i][1]); ascending i
  sample       z = seed + (3 h + t + 1) * 0x9E3779B97F4A7C15 mod 2^64; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
               z = (z ^ (z >> 27)) * 0x94D049BB133111EB; u = z ^ (z >> 31); index = ((u >> 32) * c) >> 32; two equal indices: rejected
  forms        dot (x0 y0 + x1 y1) + x2 y2; cross x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0; row times vector (r0 v0 + r1 v1) + r2 v2
  edges        s2 = s * s; for (a, b) in (0,1), (1,2), (2,0): lp = dot(p_a - p_b, p_a - p_b), lq likewise; needs lp >= s2 * lq and
               lq >= s2 * lp
  frame        u1 = p1 - p0, n1 = sqrt(dot(u1, u1)), rejected if n1 == 0, e1 = u1 / n1; w = cross(e1, p2 - p0), nw = sqrt(dot(w, w)),
               rejected if nw == 0, e3 = w / nw; e2 = cross(e3, e1); f1, f2, f3 from the q triangle in the same way
  pose         R[r][k] = (f1[r] e1[k] + f2[r] e2[k]) + f3[r] e3[k]; cp = ((p0 + p1) + p2) / 3.0, cq likewise; t = cq - R cp
  score        tau2 = tau * tau; pair i is an inlier iff dot(r, r) <= tau2 with r = (R p_i + t) - q_i; count[h] = inliers, -1: rejected
  winner       the largest count, the lowest h among equals; none accepted: best = -1, count 0, the identity pose, no flag set
"""
import functools
import math

import numpy as np

MASK = 2 ** 64 - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


# ---- matching
def dist_matrix(A, B):
    A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
    s = np.zeros((len(A), len(B)))
    for c in range(A.shape[1]):
        t = A[:, c][:, None] - B[:, c][None, :]
        s = s + t * t
    return s


def _best2(D):
    """per row of D the first two columns in the order (value, column), padded with (-1, +inf)"""
    m, n = D.shape
    idx = np.full((m, 2), -1, dtype=np.int32); d2 = np.full((m, 2), np.inf)
    k = min(n, 2)
    if m and k:
        order = np.argsort(D, axis=1, kind="stable")[:, :k]   # (stable: the lower column first among equals)
        idx[:, :k] = order
        d2[:, :k] = np.take_along_axis(D, order, 1)
    return idx, d2


def feature_match(A, B):
    """-> dict(fwd_idx (m, 2) int32, fwd_d2 (m, 2), bwd_idx (n, 2) int32, bwd_d2 (n, 2))"""
    A = np.ascontiguousarray(A, dtype=np.float64); B = np.ascontiguousarray(B, dtype=np.float64)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or not 1 <= A.shape[1] <= 64:
        raise ValueError("needs two matrices with the same 1 <= dim <= 64")
    D = dist_matrix(A, B)
    fi, fd = _best2(D)
    bi, bd = _best2(np.ascontiguousarray(D.T))
    return {"fwd_idx": fi, "fwd_d2": fd, "bwd_idx": bi, "bwd_d2": bd}


def feature_match_loop(A, B):
    m, n, dim = len(A), len(B), A.shape[1]
    a = [[float(x) for x in row] for row in A]; b = [[float(x) for x in row] for row in B]

    def dist(x, y):
        s = 0.0
        for c in range(dim):
            t = x[c] - y[c]
            s = s + t * t
        return s

    def side(X, Y):
        idx = np.full((len(X), 2), -1, dtype=np.int32); d2 = np.full((len(X), 2), np.inf)
        for i, x in enumerate(X):
            best = [(math.inf, -1), (math.inf, -1)]
            for j, y in enumerate(Y):
                d = dist(x, y)
                if best[0][1] < 0 or d < best[0][0]:          # (j ascends: a strict comparison keeps the lower j among equals)
                    best = [(d, j), best[0]]
                elif best[1][1] < 0 or d < best[1][0]:
                    best[1] = (d, j)
            for s in range(2):
                idx[i, s] = best[s][1]; d2[i, s] = best[s][0]
        return idx, d2

    fi, fd = side(a, b)
    bi, bd = side(b, a)
    return {"fwd_idx": fi, "fwd_d2": fd, "bwd_idx": bi, "bwd_d2": bd}


def match_pairs(fwd_idx, fwd_d2, bwd_idx, mutual=True, ratio=1.0):
    """-> (k, 2) int32 pairs (i, j), ascending i"""
    if not ratio > 0:
        raise ValueError("ratio must be > 0")
    fwd_idx = np.asarray(fwd_idx).reshape(-1, 2); fwd_d2 = np.asarray(fwd_d2, dtype=np.float64).reshape(-1, 2); bwd_idx = np.asarray(bwd_idx).reshape(-1, 2)
    i = np.arange(len(fwd_idx))
    j = fwd_idx[:, 0].astype(np.int64)
    keep = j >= 0
    if mutual:
        keep &= bwd_idx[np.where(keep, j, 0), 0] == i if len(bwd_idx) else False
    if not ratio >= 1:
        keep &= fwd_d2[:, 0] <= (ratio * ratio) * fwd_d2[:, 1]
    return np.ascontiguousarray(np.stack([i[keep], j[keep]], 1).astype(np.int32))


def match_pairs_loop(fwd_idx, fwd_d2, bwd_idx, mutual=True, ratio=1.0):
    out = []
    r2 = float(ratio) * float(ratio)
    for i in range(len(fwd_idx)):
        j = int(fwd_idx[i][0])
        if j < 0:
            continue
        if mutual and int(bwd_idx[j][0]) != i:
            continue
        if not ratio >= 1 and not float(fwd_d2[i][0]) <= r2 * float(fwd_d2[i][1]):
            continue
        out.append((i, j))
    return np.array(out, dtype=np.int32).reshape(-1, 2)


# ---- consensus
def sample_index(seed, h, t, c):
    z = (seed + (3 * h + t + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MIX1) & MASK
    z = ((z ^ (z >> 27)) * MIX2) & MASK
    u = z ^ (z >> 31)
    return ((u >> 32) * c) >> 32


def sample_indices(seed, H, c):
    """(H, 3) int64: the vector form of sample_index (uint64 arithmetic wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        k = (3 * np.arange(H, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]) + np.uint64(1)
        z = np.uint64(seed & MASK) + k * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        u = z ^ (z >> np.uint64(31))
        return (((u >> np.uint64(32)) * np.uint64(c)) >> np.uint64(32)).astype(np.int64)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _frames(T):
    """T (H, 3, 3): triangles -> (ok (H,), e1, e2, e3)"""
    u1 = T[:, 1] - T[:, 0]
    n1 = np.sqrt(_dot(u1, u1))
    e1 = u1 / n1[:, None]
    w = _cross(e1, T[:, 2] - T[:, 0])
    nw = np.sqrt(_dot(w, w))
    e3 = w / nw[:, None]
    e2 = _cross(e3, e1)
    return ~(n1 == 0) & ~(nw == 0), e1, e2, e3


def hypotheses(P, Q, H, seed, edge_sim=0.9):
    """-> (accepted (H,) bool, R (H, 3, 3), t (H, 3), idx (H, 3)); R and t of a rejected hypothesis mean nothing"""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3); Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    c = len(P)
    idx = sample_indices(seed, H, c)
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 2] != idx[:, 0])
    TP, TQ = P[idx], Q[idx]
    s2 = edge_sim * edge_sim
    with np.errstate(all="ignore"):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            dp, dq = TP[:, a] - TP[:, b], TQ[:, a] - TQ[:, b]
            lp, lq = _dot(dp, dp), _dot(dq, dq)
            ok &= (lp >= s2 * lq) & (lq >= s2 * lp)
        okp, e1, e2, e3 = _frames(TP)
        okq, f1, f2, f3 = _frames(TQ)
        ok &= okp & okq
        R = (f1[:, :, None] * e1[:, None, :] + f2[:, :, None] * e2[:, None, :]) + f3[:, :, None] * e3[:, None, :]
        cp = ((TP[:, 0] + TP[:, 1]) + TP[:, 2]) / 3.0
        cq = ((TQ[:, 0] + TQ[:, 1]) + TQ[:, 2]) / 3.0
        Rcp = (R[:, :, 0] * cp[:, None, 0] + R[:, :, 1] * cp[:, None, 1]) + R[:, :, 2] * cp[:, None, 2]
        t = cq - Rcp
    return ok, R, t, idx


def _inliers(R, t, P, Q, tau2):
    """R (A, 3, 3), t (A, 3) -> (A, c) bool"""
    with np.errstate(all="ignore"):
        r = []
        for k in range(3):
            y = (R[:, k, 0][:, None] * P[None, :, 0] + R[:, k, 1][:, None] * P[None, :, 1]) + R[:, k, 2][:, None] * P[None, :, 2]
            r.append((y + t[:, k][:, None]) - Q[None, :, k])
        return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2] <= tau2


def consensus(P, Q, H, seed, tau, edge_sim=0.9):
    """-> dict(best, count, accepted, pose (4, 4), counts (H,) int32, flags (c,) uint8)"""
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(-1, 3); Q = np.ascontiguousarray(Q, dtype=np.float64).reshape(-1, 3)
    if len(P) < 3 or len(P) != len(Q) or not 1 <= H <= 2 ** 24 or not (tau > 0 and math.isfinite(tau)) or not 0 <= edge_sim < 1:
        raise ValueError("needs c >= 3, 1 <= H <= 2^24, a finite tau > 0 and 0 <= edge_sim < 1")
    ok, R, t, _ = hypotheses(P, Q, H, seed, edge_sim)
    tau2 = tau * tau
    counts = np.full(H, -1, dtype=np.int32)
    acc = np.flatnonzero(ok)
    for lo in range(0, len(acc), 2048):
        part = acc[lo:lo + 2048]
        counts[part] = _inliers(R[part], t[part], P, Q, tau2).sum(1)
    pose = np.eye(4); flags = np.zeros(len(P), dtype=np.uint8)
    best, count = -1, 0
    if len(acc):
        best = int(np.argmax(counts))     # (the first of the largest: the lowest h)
        count = int(counts[best])
        pose[:3, :3] = R[best]; pose[:3, 3] = t[best]
        flags = _inliers(R[best:best + 1], t[best:best + 1], P, Q, tau2)[0].astype(np.uint8)
    return {"best": best, "count": count, "accepted": int(len(acc)), "pose": pose, "counts": counts, "flags": flags}


def consensus_loop(P, Q, H, seed, tau, edge_sim=0.9):
    P = [[float(x) for x in row] for row in P]; Q = [[float(x) for x in row] for row in Q]
    c = len(P)

    def sub(a, b):
        return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def frame(T):
        u1 = sub(T[1], T[0])
        n1 = math.sqrt(dot(u1, u1))
        if n1 == 0:
            return None
        e1 = [u1[0] / n1, u1[1] / n1, u1[2] / n1]
        w = cross(e1, sub(T[2], T[0]))
        nw = math.sqrt(dot(w, w))
        if nw == 0:
            return None
        e3 = [w[0] / nw, w[1] / nw, w[2] / nw]
        return e1, cross(e3, e1), e3

    def pose_of(h):
        ids = [sample_index(seed, h, t, c) for t in range(3)]
        if ids[0] == ids[1] or ids[1] == ids[2] or ids[2] == ids[0]:
            return None
        TP, TQ = [P[i] for i in ids], [Q[i] for i in ids]
        s2 = edge_sim * edge_sim
        for a, b in ((0, 1), (1, 2), (2, 0)):
            dp, dq = sub(TP[a], TP[b]), sub(TQ[a], TQ[b])
            lp, lq = dot(dp, dp), dot(dq, dq)
            if not (lp >= s2 * lq and lq >= s2 * lp):
                return None
        fp, fq = frame(TP), frame(TQ)
        if fp is None or fq is None:
            return None
        (e1, e2, e3), (f1, f2, f3) = fp, fq
        R = [[(f1[r] * e1[k] + f2[r] * e2[k]) + f3[r] * e3[k] for k in range(3)] for r in range(3)]
        cp = [((TP[0][k] + TP[1][k]) + TP[2][k]) / 3.0 for k in range(3)]
        cq = [((TQ[0][k] + TQ[1][k]) + TQ[2][k]) / 3.0 for k in range(3)]
        t = [cq[r] - dot(R[r], cp) for r in range(3)]
        return R, t

    tau2 = tau * tau

    def inlier(R, t, i):
        r = [(dot(R[k], P[i]) + t[k]) - Q[i][k] for k in range(3)]
        return dot(r, r) <= tau2

    counts = np.full(H, -1, dtype=np.int32)
    best, count, accepted, best_pose = -1, 0, 0, None
    for h in range(H):
        rt = pose_of(h)
        if rt is None:
            continue
        accepted += 1
        n = sum(1 for i in range(c) if inlier(rt[0], rt[1], i))
        counts[h] = n
        if best < 0 or n > count:
            best, count, best_pose = h, n, rt
    pose = np.eye(4); flags = np.zeros(c, dtype=np.uint8)
    if best >= 0:
        pose[:3, :3] = np.array(best_pose[0]); pose[:3, 3] = np.array(best_pose[1])
        flags = np.array([1 if inlier(best_pose[0], best_pose[1], i) else 0 for i in range(c)], dtype=np.uint8)
    return {"best": best, "count": count, "accepted": accepted, "pose": pose, "counts": counts, "flags": flags}


def same(a, b, keys):
    """Byte equality of two results over `keys` (arrays by dtype, shape and bytes; scalars by value)."""
    for key in keys:
        x, y = a[key], b[key]
        if isinstance(x, (int, np.integer)) and isinstance(y, (int, np.integer)):
            if int(x) != int(y):
                return False
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


MATCH_KEYS = ("fwd_idx", "fwd_d2", "bwd_idx", "bwd_d2")
CONSENSUS_KEYS = ("best", "count", "accepted", "pose", "counts", "flags")


# ---- the test cloud
@functools.lru_cache(maxsize=None)
def _bump_field():
    rng = np.random.Generator(np.random.PCG64(1))
    c = rng.uniform(0.0, 1.0, size=(40, 2))
    a = rng.uniform(-0.06, 0.06, size=40)
    s = rng.uniform(0.03, 0.07, size=40)
    return c, a, s


def bumps(n, seed, lo=0.0, hi=1.0):
    """n points of the height field z = sum_k a_k exp(-|xy - c_k|^2 / 2 sigma_k^2) of 40 bumps (drawn once from PCG64(1): c ~ U(0,1)^2,
    then a ~ U(-0.06, 0.06), then sigma ~ U(0.03, 0.07)), sampled at x ~ U(lo, hi), then y ~ U(0, 1) from PCG64(seed), with the analytic
    unit normals (-z_x, -z_y, 1) / |.|.  -> (points (n, 3), normals (n, 3)).  Rough at the neighbourhood scale and without symmetry:
    descriptors discriminate and the pose is unambiguous."""
    c, a, s = _bump_field()
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(lo, hi, size=n)
    y = rng.uniform(0.0, 1.0, size=n)
    dx, dy = x[:, None] - c[None, :, 0], y[:, None] - c[None, :, 1]
    g = a[None, :] * np.exp(-(dx * dx + dy * dy) / (2.0 * s[None, :] ** 2))
    z = g.sum(1)
    zx, zy = (g * (-dx / s[None, :] ** 2)).sum(1), (g * (-dy / s[None, :] ** 2)).sum(1)
    nrm = np.stack([-zx, -zy, np.ones(n)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(np.stack([x, y, z], 1)), np.ascontiguousarray(nrm)


# ---- the end-to-end case of tests/test_match_cpu.py and tests/test_gpu_match.py
E2E_W, E2E_T = (0.7, -1.1, 0.4), (0.3, -0.2, 0.5)
E2E_H, E2E_SEED, E2E_EDGE_SIM, E2E_MAX_NN = 8000, 12345, 0.9, 64


@functools.lru_cache(maxsize=None)
def e2e_clouds(partial=False):
    """-> dict(src, src_nrm, dst, dst_nrm, truth (4, 4): src -> dst, spacing, radius, tau).  src = bumps(1500, 100); dst = another
    sampling of the same surface (bumps(1500, 200), or over x in [0.3, 1.3] for the partial-overlap pair) moved by the true pose; radius =
    the median distance from a point of src to its 60th neighbour, spacing = the median distance to its nearest, tau = 2 spacings."""
    import knnref
    from mvicp import synth
    src, src_n = bumps(1500, 100)
    d, d_n = bumps(1500, 200, 0.3, 1.3) if partial else bumps(1500, 200)
    R = synth.so3_exp(np.array(E2E_W)); t = np.array(E2E_T)
    dst, dst_n = np.ascontiguousarray(d @ R.T + t), np.ascontiguousarray(d_n @ R.T)
    truth = np.eye(4); truth[:3, :3] = R; truth[:3, 3] = t
    _, Ds = knnref.sorted_rows(src)         # (column 0 is the point itself)
    spacing = float(np.median(np.sqrt(Ds[:, 1])))
    radius = float(np.median(np.sqrt(Ds[:, 60])))
    return {"src": src, "src_nrm": src_n, "dst": dst, "dst_nrm": dst_n, "truth": truth, "spacing": spacing, "radius": radius, "tau": 2.0 * spacing}


@functools.lru_cache(maxsize=None)
def e2e_reference(partial=False):
    """The whole chain on the CPU: fpfhref descriptors of both clouds -> feature_match -> match_pairs (mutual, no ratio test) -> consensus.
    -> dict(desc_src, desc_dst, match, pairs, consensus, P, Q)"""
    import fpfhref
    cl = e2e_clouds(partial)
    da = fpfhref.fpfh(cl["src"], cl["src_nrm"], cl["radius"], E2E_MAX_NN)["desc"]
    db = fpfhref.fpfh(cl["dst"], cl["dst_nrm"], cl["radius"], E2E_MAX_NN)["desc"]
    mt = feature_match(da, db)
    pairs = match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], True, 1.0)
    P, Q = np.ascontiguousarray(cl["src"][pairs[:, 0]]), np.ascontiguousarray(cl["dst"][pairs[:, 1]])
    cons = consensus(P, Q, E2E_H, E2E_SEED, cl["tau"], E2E_EDGE_SIM)
    return {"desc_src": da, "desc_dst": db, "match": mt, "pairs": pairs, "consensus": cons, "P": P, "Q": Q}


def pose_error(pose, truth):
    """-> (rotation angle in degrees, |translation difference|) between two 4 x 4 poses"""
    from mvicp import synth
    dt, ang = synth.pose_diff(np.asarray(pose), np.asarray(truth))
    return math.degrees(ang), dt
