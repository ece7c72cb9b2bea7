"""The contract of mvicp_segment_plane, mvicp_plane_select and mvicp_plane_from_moments (include/mvicp.h) in numpy (`segment`,
`from_moments`, `select`), and the same statement as a plain Python loop over scalar floats and ints (`segment_loop`).  fp64 throughout,
every operation rounded on its own (numpy never contracts to fma); the integer sums are exact (int64, then Python ints for the 128-bit
products).

  sample     hypothesis h, slot t: matchref.sample_index(seed, h, t, n); two equal indices: rejected (before any load)
  plane      a = p[i0], u = p[i1] - a, v = p[i2] - a, w = cross(u, v), nw = sqrt(dot(w, w)); rejected unless 0 < nw < +inf; m = w / nw
  direction  (axis given) da = dot(m, axis); rejected unless da * da >= (cos_min * cos_min) * dot(axis, axis)
  score      o_i = p_i - a, r_i = dot(m, o_i); inlier iff fabs(r_i) <= tau; count[h] = inliers, -1: rejected
  winner     the largest count, the lowest h among equals; none accepted: best = -1, count 0, an all-zero plane, no flag set
  refit      over the winner's inliers (c of them): omax = max |o_ik|; omax == 0: refused.  L = bit length of c, b = min(21, (62 - L) // 2),
             q with 2^(b-1) <= omax 2^q < 2^b, M_i = floor(ldexp(o_i, q)), s = sum M, S = sum M M^T (int64), C = c S - s s^T (128 bits ->
             double, nearest even), normref._jacobi on C with V = I, the column of the smallest diagonal entry (two strict comparisons)
             divided by its length, negated iff its dot product with m is < 0 -> m'; g = a + ldexp(s / c + 0.5, -q); flags and
             count_refined by fabs(dot(m', p_i - g)) <= tau
  forms      dot (x0 y0 + x1 y1) + x2 y2; cross x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0 (those of mvicp_consensus)
"""
import functools
import math

import numpy as np

import matchref
import normref

RECORD_INTS = ("best", "count", "accepted", "refit", "count_refined", "b", "q", "n", "has_normals")
RECORD_VECS = ("normal", "point", "d", "hyp_normal", "hyp_point")


def check_args(tau, H, axis, cos_min):
    if not (math.isfinite(tau) and tau > 0):
        raise ValueError("tau must be finite and > 0")
    if not 1 <= H <= 2 ** 24:
        raise ValueError("needs 1 <= hypotheses <= 2^24")
    if axis is None:
        return None
    ax = np.asarray(axis, dtype=np.float64).reshape(3)
    if not np.isfinite(ax).all() or not ax.any():
        raise ValueError("axis must be finite and not all zero")
    if not 0 <= cos_min <= 1:
        raise ValueError("needs 0 <= cos_min <= 1")
    return ax


def bit_rule(c, omax):
    """-> (b, q) of a refit over c inliers whose largest |offset| is omax > 0"""
    L = int(c).bit_length()
    b = min(21, (62 - L) // 2)
    _, ex = math.frexp(omax)   # omax = f 2^ex, f in [0.5, 1)
    return b, b - ex


def moments(o, q):
    """The ten integers of the offsets o (c, 3) at the scale 2^q -> (s [3], S [6]: 00 01 02 11 12 22) as Python ints (exact int64 sums)."""
    M = np.floor(np.ldexp(o, q)).astype(np.int64)
    s = [int(M[:, k].sum()) for k in range(3)]
    S = [int((M[:, k] * M[:, l]).sum()) for k in range(3) for l in range(k, 3)]
    return s, S


def from_moments(c, s, S, q, a, m):
    """The refit rule from the integer sums on (mvicp_plane_from_moments) -> (normal (3,), point (3,))"""
    idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
    A = np.zeros((1, 3, 3))
    for k in range(3):
        for l in range(k, 3):
            A[0, k, l] = A[0, l, k] = float(int(c) * int(S[idx[(k, l)]]) - int(s[k]) * int(s[l]))   # (Python int -> float: nearest even)
    V = np.zeros((1, 3, 3)); V[0, 0, 0] = V[0, 1, 1] = V[0, 2, 2] = 1.0
    A, V = normref._jacobi(A, V)
    j = 0
    if A[0, 1, 1] < A[0, j, j]:
        j = 1
    if A[0, 2, 2] < A[0, j, j]:
        j = 2
    v = V[0, :, j]
    with np.errstate(all="ignore"):
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nv = v / ln
        m = np.asarray(m, dtype=np.float64)
        if (nv[0] * m[0] + nv[1] * m[1]) + nv[2] * m[2] < 0:
            nv = -nv
        a = np.asarray(a, dtype=np.float64)
        g = np.array([a[k] + np.ldexp(np.float64(float(int(s[k]))) / np.float64(float(int(c))) + 0.5, -int(q)) for k in range(3)])
    return np.ascontiguousarray(nv), g


def _empty(n, H, has_normals):
    z = np.zeros(3)
    return {"best": -1, "count": 0, "accepted": 0, "refit": 0, "count_refined": 0, "b": 0, "q": 0, "n": n, "has_normals": int(has_normals),
            "normal": z.copy(), "point": z.copy(), "d": 0.0, "hyp_normal": z.copy(), "hyp_point": z.copy(),
            "counts": np.full(H, -1, dtype=np.int32), "flags": np.zeros(n, dtype=np.uint8), "moments": None}


def _plane_d(nv, g):
    return -float((nv[0] * g[0] + nv[1] * g[1]) + nv[2] * g[2])


def hypotheses(p, H, seed, axis=None, cos_min=0.0):
    """-> (accepted (H,) bool, a (H, 3), m (H, 3)); a and m of a rejected hypothesis mean nothing"""
    n = len(p)
    idx = matchref.sample_indices(seed, H, n)
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 2] != idx[:, 0])
    if n == 0:
        return np.zeros(H, dtype=bool), np.zeros((H, 3)), np.zeros((H, 3))
    with np.errstate(all="ignore"):
        a = p[idx[:, 0]]
        w = matchref._cross(p[idx[:, 1]] - a, p[idx[:, 2]] - a)
        nw = np.sqrt(matchref._dot(w, w))
        ok &= (nw > 0) & (nw < np.inf)
        m = w / nw[:, None]
        if axis is not None:
            da = matchref._dot(m, axis[None, :])
            ok &= da * da >= (cos_min * cos_min) * float((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2])
    return ok, a, m


def _residual(m, a, p):
    """m, a (A, 3), p (n, 3) -> (A, n)"""
    with np.errstate(all="ignore"):
        o = p[None, :, :] - a[:, None, :]
        return (m[:, 0][:, None] * o[:, :, 0] + m[:, 1][:, None] * o[:, :, 1]) + m[:, 2][:, None] * o[:, :, 2]


def segment(p, nrm, tau, H=1024, seed=0, axis=None, cos_min=0.0, refine=True):
    """-> dict(the record's fields, counts (H,) int32, flags (n,) uint8, moments: (c, s, S, q, a, m) of a refit or None)"""
    ax = check_args(tau, H, axis, cos_min)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    R = _empty(n, H, nrm is not None)
    ok, a, m = hypotheses(p, H, seed, ax, cos_min)
    acc = np.flatnonzero(ok)
    R["accepted"] = int(len(acc))
    if not len(acc):
        return R
    step = max(1, (1 << 22) // max(n, 1))
    for lo in range(0, len(acc), step):
        part = acc[lo:lo + step]
        R["counts"][part] = (np.abs(_residual(m[part], a[part], p)) <= tau).sum(1)
    best = int(np.argmax(R["counts"]))   # (the first of the largest: the lowest h)
    ab, mb = a[best].copy(), m[best].copy()
    flags = np.abs(_residual(mb[None], ab[None], p))[0] <= tau
    c = int(flags.sum())
    assert c == int(R["counts"][best])
    R.update(best=best, count=c, count_refined=c, normal=mb.copy(), point=ab.copy(), hyp_normal=mb, hyp_point=ab, d=_plane_d(mb, ab))
    if refine:
        o = p[flags] - ab
        omax = float(np.abs(o).max())
        if omax > 0:
            b, q = bit_rule(c, omax)
            s, S = moments(o, q)
            nv, g = from_moments(c, s, S, q, ab, mb)
            with np.errstate(all="ignore"):
                flags = np.abs(_residual(nv[None], g[None], p))[0] <= tau
            R.update(refit=1, b=b, q=q, normal=nv, point=g, d=_plane_d(nv, g), count_refined=int(flags.sum()), moments=(c, s, S, q, ab, mb))
    R["flags"] = flags.astype(np.uint8)
    return R


def segment_loop(p, nrm, tau, H=1024, seed=0, axis=None, cos_min=0.0, refine=True):
    """The same contract, one scalar operation at a time on Python floats and ints."""
    ax = check_args(tau, H, axis, cos_min)
    P = [[float(x) for x in row] for row in np.asarray(p, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    R = _empty(n, H, nrm is not None)
    tau = float(tau)
    INF = float("inf")

    def sub(x, y):
        return [x[0] - y[0], x[1] - y[1], x[2] - y[2]]

    def dot(x, y):
        return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]

    def cross(x, y):
        return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]

    def div(x, y):   # IEEE division of floats, y != 0
        return float(np.float64(x) / np.float64(y))

    def plane_of(h):
        i0, i1, i2 = (matchref.sample_index(seed, h, t, n) for t in range(3))
        if i0 == i1 or i1 == i2 or i2 == i0:
            return None
        a = P[i0]
        w = cross(sub(P[i1], a), sub(P[i2], a))
        ww = dot(w, w)
        nw = math.sqrt(ww) if ww >= 0 else float("nan")   # (a NaN fails both comparisons)
        if not (0 < nw < INF):
            return None
        m = [div(w[k], nw) for k in range(3)]
        if ax is not None:
            A = [float(v) for v in ax]
            da = dot(m, A)
            if not da * da >= (float(cos_min) * float(cos_min)) * dot(A, A):
                return None
        return a, m

    def inlier(m, g, i):
        return abs(dot(m, sub(P[i], g))) <= tau

    best, count, plane = -1, 0, None
    for h in range(H):
        am = plane_of(h)
        if am is None:
            continue
        R["accepted"] += 1
        k = sum(1 for i in range(n) if inlier(am[1], am[0], i))
        R["counts"][h] = k
        if best < 0 or k > count:
            best, count, plane = h, k, am
    if best < 0:
        return R
    a, m = plane
    flags = [inlier(m, a, i) for i in range(n)]
    R.update(best=best, count=count, count_refined=count, normal=np.array(m), point=np.array(a), hyp_normal=np.array(m), hyp_point=np.array(a),
             d=-dot(m, a))
    if refine:
        omax = 0.0
        for i in range(n):
            if flags[i]:
                omax = max([omax] + [abs(v) for v in sub(P[i], a)])
        if omax > 0:
            b, q = bit_rule(count, omax)
            s, S = [0, 0, 0], [0] * 6
            for i in range(n):
                if flags[i]:
                    M = [int(math.floor(math.ldexp(v, q))) for v in sub(P[i], a)]
                    t = 0
                    for k in range(3):
                        s[k] += M[k]
                        for l in range(k, 3):
                            S[t] += M[k] * M[l]; t += 1
            nv, g = from_moments(count, s, S, q, a, m)
            nv, g = [float(v) for v in nv], [float(v) for v in g]
            flags = [inlier(nv, g, i) for i in range(n)]
            R.update(refit=1, b=b, q=q, normal=np.array(nv), point=np.array(g), d=-dot(nv, g), count_refined=sum(flags), moments=(count, s, S, q, a, m))
    R["flags"] = np.array(flags, dtype=np.uint8).reshape(n)
    return R


def select(p, nrm, res, inliers=True):
    """The rows with flag = 1 (inliers) or flag = 0, in ascending original index -> dict(xyz, nrm or None, idx int32, kept)."""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    idx = np.flatnonzero(res["flags"] == (1 if inliers else 0)).astype(np.int32)
    return {"xyz": p[idx], "nrm": None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float64)[idx], "idx": idx, "kept": len(idx)}


def _bytes_equal(x, y, dt):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == dt and y.dtype == dt and x.shape == y.shape and x.tobytes() == y.tobytes()


def same(a, b):
    """Byte equality of two results: the record, the counts and the flags (signs of zeros included)."""
    if not all(int(a[k]) == int(b[k]) for k in RECORD_INTS):
        return False
    if not all(_bytes_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), np.float64) for k in RECORD_VECS):
        return False
    return _bytes_equal(a["counts"], b["counts"], np.int32) and _bytes_equal(a["flags"], b["flags"], np.uint8)


def same_kept(a, b):
    """Byte equality of two selections."""
    if (a["nrm"] is None) != (b["nrm"] is None) or int(a["kept"]) != int(b["kept"]):
        return False
    if a["nrm"] is not None and not _bytes_equal(a["nrm"], b["nrm"], np.float64):
        return False
    return _bytes_equal(a["xyz"], b["xyz"], np.float64) and _bytes_equal(a["idx"], b["idx"], np.int32)


# ---- the clouds of the tests
def _unit_normals(rng, n):
    nr = rng.normal(size=(n, 3))
    return nr / np.linalg.norm(nr, axis=1, keepdims=True)


NOISY_TAU = 0.006
NOISY_NORMAL = np.array([0.2, -0.3, 1.0]) / math.sqrt(1.13)
NOISY_ORIGIN = np.array([0.1, -0.2, 0.3])


@functools.lru_cache(maxsize=None)
def noisy_plane_cloud():
    """2 000 points of the plane through NOISY_ORIGIN with the unit normal NOISY_NORMAL (uniform over a 1 x 1 patch, sigma = 2 mm along the
    normal), 600 uniform clutter points in the 1.2-cube around it and a 40-point clump (sigma 4 mm) 15 cm above the plane, shuffled
    -> (points, unit normals, mask of the plane points)."""
    rng = np.random.Generator(np.random.PCG64(1907))
    e1 = np.cross(NOISY_NORMAL, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(NOISY_NORMAL, e1)
    uv = rng.uniform(-0.5, 0.5, size=(2000, 2))
    plane = NOISY_ORIGIN + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0.0, 0.002, size=(2000, 1)) * NOISY_NORMAL
    clutter = NOISY_ORIGIN + rng.uniform(-0.6, 0.6, size=(600, 3))
    clump = NOISY_ORIGIN + 0.15 * NOISY_NORMAL + rng.normal(0.0, 0.004, size=(40, 3))
    p = np.concatenate([plane, clutter, clump], 0)
    perm = rng.permutation(len(p))
    mask = np.zeros(len(p), dtype=bool); mask[:2000] = True
    return np.ascontiguousarray(p[perm]), _unit_normals(rng, len(p)), mask[perm]


SLAB_PITCH = 2.0 ** -8


@functools.lru_cache(maxsize=None)
def dyadic_slab():
    """16 x 16 x 3 points at pitch 2^-8, shuffled: every coordinate and difference is exact, so |r| == tau can hold exactly."""
    p = np.array([[x, y, z] for z in range(3) for y in range(16) for x in range(16)], dtype=np.float64) * SLAB_PITCH
    return np.ascontiguousarray(p[np.random.Generator(np.random.PCG64(1902)).permutation(len(p))])


FLOOR_WALL_TAU = 0.005


@functools.lru_cache(maxsize=None)
def floor_wall_cloud():
    """A floor (z = 0, 1 500 points over [0, 1]^2) and a wall (x = 0, 2 500 points over y in [0, 1], z in [0, 1]), sigma 1 mm each,
    shuffled -> (points, mask of the floor points)."""
    rng = np.random.Generator(np.random.PCG64(1903))
    floor = np.column_stack([rng.uniform(0.0, 1.0, 1500), rng.uniform(0.0, 1.0, 1500), rng.normal(0.0, 0.001, 1500)])
    wall = np.column_stack([rng.normal(0.0, 0.001, 2500), rng.uniform(0.0, 1.0, 2500), rng.uniform(0.0, 1.0, 2500)])
    p = np.concatenate([floor, wall], 0)
    perm = rng.permutation(len(p))
    mask = np.zeros(len(p), dtype=bool); mask[:1500] = True
    return np.ascontiguousarray(p[perm]), mask[perm]


TABLE_TAU, TABLE_RADIUS, TABLE_MIN_PTS = 0.004, 0.04, 4


@functools.lru_cache(maxsize=None)
def tabletop_cloud():
    """A floor (a jittered 36 x 36 grid over [0, 0.9]^2, sigma 1 mm in z) with two boxes standing on it (0.15 x 0.15 x 0.2, 350 surface
    points each, the lowest 1 cm above the floor, 0.35 apart), shuffled -> (points, part: 0 floor, 1 and 2 the boxes)."""
    rng = np.random.Generator(np.random.PCG64(1904))
    gx, gy = np.meshgrid(np.arange(36) * 0.025, np.arange(36) * 0.025)
    floor = np.column_stack([gx.ravel() + rng.uniform(0, 0.01, 1296), gy.ravel() + rng.uniform(0, 0.01, 1296), rng.normal(0.0, 0.001, 1296)])

    def box(x0, y0):
        q = rng.uniform(0.0, 1.0, size=(350, 3)) * [0.15, 0.15, 0.19] + [x0, y0, 0.01]
        face = rng.integers(0, 5, size=350)   # four sides and the top
        q[face == 0, 0] = x0; q[face == 1, 0] = x0 + 0.15; q[face == 2, 1] = y0; q[face == 3, 1] = y0 + 0.15; q[face == 4, 2] = 0.2
        return q
    p = np.concatenate([floor, box(0.15, 0.4), box(0.6, 0.4)], 0)
    part = np.concatenate([np.zeros(1296, np.int32), np.full(350, 1, np.int32), np.full(350, 2, np.int32)])
    perm = rng.permutation(len(p))
    return np.ascontiguousarray(p[perm]), part[perm]


def line_cloud():
    """400 points on a line along x, off the origin, shuffled (clusterref.line_cloud): every cross product of two differences is exactly zero."""
    import clusterref
    return clusterref.line_cloud()


def dyadic_plane(n):
    """n points of the plane z = 2^-3 on a 2^-12 lattice (x fastest, 2048 per row): every offset, product and sum of the refit is exact."""
    i = np.arange(n, dtype=np.int64)
    return np.ascontiguousarray(np.column_stack([(i % 2048) * 2.0 ** -12, (i // 2048) * 2.0 ** -12, np.full(n, 0.125)]))
