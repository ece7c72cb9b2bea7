"""The contract of mvicp_iss_keypoints (include/mvicp.h) in numpy (`iss`), and the same statement as a plain Python loop over scalar
ints and floats (`iss_loop`).  Intrinsic Shape Signatures (Zhong 2009): the eigenvalues l1 >= l2 >= l3 of the covariance of a point's
neighbourhood, salient iff l2 / l1 and l3 / l2 are below their thresholds, keypoint iff no neighbour within the second radius has a
larger l3.  What makes it a pure function of the stored bytes: the neighbourhood is the candidate set of a self-mode mvicp_knn_search row
(sqrt(dist2) < r), the moments are sums of INTEGERS g = floor((p_j - p_i) 2^q) -- so the order of the neighbours is free --, the
eigenvalues come from a fixed number of Jacobi sweeps in stated operations, and ties of the suppression go to the lowest index.

Every integer stays below 2^62 (asserted on every call).  |g| <= 2^20 + 1: sqrt(dist2) < r gives |p_j - p_i| < r per component up to one
rounding, r 2^q = f 2^20 with f < 1, and floor moves a value by less than 1.  With c <= 1024 = 2^10 neighbours: |m_a| <= c (2^20 + 1) <
2^31, S_ab <= c (2^20 + 1)^2 < 2^51, so c S_ab < 2^61 and |m_a m_b| < 2^62; D_aa = c S_aa - m_a^2 lies in [0, c S_aa] (Cauchy-Schwarz)
and |D_ab| <= sqrt(D_aa D_bb) < 2^61."""
import bisect
import math

import numpy as np

import knnref

CAP = 1024          # neighbours of a salient row
BITS = 20
SWEEPS = 6
PAIRS = ((0, 1), (0, 2), (1, 2))
LIMIT = 1 << 62


class TooManyNeighbours(ValueError):
    """a salient neighbourhood of more than CAP points: the library reports MVICP_ERR_ARG"""


def check_args(salient_radius, non_max_radius, gamma21, gamma32, min_neighbors):
    for r in (salient_radius, non_max_radius):
        if not (math.isfinite(r) and 2.0 ** -300 <= r <= 2.0 ** 300):
            raise ValueError("a radius must be finite and lie in [2^-300, 2^300]")
    for g in (gamma21, gamma32):
        if not (math.isfinite(g) and g > 0):
            raise ValueError("gamma21 and gamma32 must be finite and > 0")
    if not 1 <= min_neighbors <= CAP:
        raise ValueError("needs 1 <= min_neighbors <= 1024")


def q_exponent(salient_radius):
    """salient_radius = f 2^e with f in [0.5, 1): q = 20 - e, so that radius 2^q = f 2^20"""
    return BITS - math.frexp(salient_radius)[1]


def _jacobi(A):
    """SWEEPS sweeps over PAIRS on the (n, 3, 3) stack A, in place; a rotation is skipped iff A[p][q] == 0"""
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in PAIRS:
                on = A[:, p, q] != 0
                theta = (A[:, q, q] - A[:, p, p]) / (2.0 * A[:, p, q])
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                B = A.copy()
                for r in range(3):
                    arp, arq = B[:, r, p].copy(), B[:, r, q].copy()
                    B[:, r, p] = c * arp - s * arq; B[:, r, q] = s * arp + c * arq
                for r in range(3):
                    apr, aqr = B[:, p, r].copy(), B[:, q, r].copy()
                    B[:, p, r] = c * apr - s * aqr; B[:, q, r] = s * apr + c * aqr
                A[on] = B[on]
    return A


def iss(p, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """-> dict(idx (k,) int32 ascending, xyz (k, 3), saliency (n,), cnt_salient (n,) int32, cnt_nms (n,) int32) and, for the tests, eig
    (n, 3) = (l1, l2, l3) in units of 2^-2q, salient (n,) bool, beaten (n,) bool, tied (n,) bool: a neighbour of the second radius has
    exactly the point's own positive saliency."""
    check_args(salient_radius, non_max_radius, gamma21, gamma32, min_neighbors)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    q = q_exponent(salient_radius)
    scale, unscale = math.ldexp(1.0, q), math.ldexp(1.0, -2 * q)
    cs, m, S = np.zeros(n, dtype=np.int64), np.zeros((n, 3), dtype=np.int64), np.zeros((n, 3, 3), dtype=np.int64)
    near = []
    for a in range(0, n, 256):
        sl = slice(a, a + 256)
        dist = np.sqrt(knnref.dist2_matrix(p[sl], p))
        in_s = dist < salient_radius
        near.append(dist < non_max_radius)
        cs[sl] = in_s.sum(1)
        if (cs[sl] > CAP).any():
            raise TooManyNeighbours("%d points within the salient radius of one point" % cs[sl].max())
        g = np.floor((p[None, :, :] - p[sl, None, :]) * scale)
        g = np.where(in_s[:, :, None], g, 0.0).astype(np.int64)
        assert (np.abs(g) <= (1 << BITS) + 1).all()
        m[sl] = g.sum(1)
        S[sl] = np.einsum("ija,ijb->iab", g, g)
    c = cs[:, None, None]
    assert (np.abs(c * S) < LIMIT).all() and (np.abs(m[:, :, None] * m[:, None, :]) < LIMIT).all()
    D = c * S - m[:, :, None] * m[:, None, :]
    assert (np.abs(D) < LIMIT).all()
    C = D.astype(np.float64) / (cs * cs).astype(np.float64)[:, None, None] if n else np.zeros((0, 3, 3))
    A = _jacobi(C.copy())
    eig = -np.sort(-np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1), axis=1) if n else np.zeros((0, 3))
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    salient = (cs >= min_neighbors) & (l2 < gamma21 * l1) & (l3 < gamma32 * l2) & (l3 > 0)
    sal = np.where(salient, l3 * unscale, 0.0)
    cn, beaten, tied = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    ar = np.arange(n)
    for a, nb in zip(range(0, n, 256), near):
        sl = slice(a, a + 256)
        cn[sl] = nb.sum(1)
        eq = nb & (sal[None, :] == sal[sl, None])
        beaten[sl] = (nb & (sal[None, :] > sal[sl, None])).any(1) | (eq & (ar[None, :] < ar[sl, None])).any(1)
        tied[sl] = (eq & (ar[None, :] != ar[sl, None])).any(1) & (sal[sl] > 0)
    key = (sal > 0) & (cn >= min_neighbors) & ~beaten
    idx = np.nonzero(key)[0].astype(np.int32)
    return {"idx": idx, "xyz": np.ascontiguousarray(p[idx]), "saliency": np.ascontiguousarray(sal), "cnt_salient": cs.astype(np.int32),
            "cnt_nms": cn.astype(np.int32), "eig": eig, "salient": salient, "beaten": beaten, "tied": tied, "q": q}


def _jacobi_scalar(A):
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            if A[p][q] == 0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for r in range(3):
                arp, arq = A[r][p], A[r][q]
                A[r][p] = c * arp - s * arq; A[r][q] = s * arp + c * arq
            for r in range(3):
                apr, aqr = A[p][r], A[q][r]
                A[p][r] = c * apr - s * aqr; A[q][r] = s * apr + c * aqr
    return A


def iss_loop(p, salient_radius, non_max_radius, gamma21=0.975, gamma32=0.975, min_neighbors=5):
    """The same contract, one scalar operation at a time: Python ints for the moments, Python floats for the rest.  The only shortcut is
    which pairs are LOOKED at: the points are walked in the order of their x, and a pair whose x differ by more than 1.001 radii is not
    within the radius (|dx| <= sqrt(dist2) up to two roundings)."""
    check_args(salient_radius, non_max_radius, gamma21, gamma32, min_neighbors)
    P = [[float(v) for v in row] for row in np.asarray(p, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    q = q_exponent(salient_radius)
    scale, unscale = math.ldexp(1.0, q), math.ldexp(1.0, -2 * q)
    by_x = sorted(range(n), key=lambda i: P[i][0])
    xs = [P[i][0] for i in by_x]

    def neighbours(i, radius):
        lo, hi = bisect.bisect_left(xs, P[i][0] - 1.001 * radius), bisect.bisect_right(xs, P[i][0] + 1.001 * radius)
        out = []
        for j in by_x[lo:hi]:
            d0, d1, d2 = P[i][0] - P[j][0], P[i][1] - P[j][1], P[i][2] - P[j][2]
            if math.sqrt((d0 * d0 + d1 * d1) + d2 * d2) < radius:
                out.append(j)
        return out

    sal, cs, eig = [0.0] * n, [0] * n, []
    for i in range(n):
        nb = neighbours(i, salient_radius)
        c = len(nb)
        if c > CAP:
            raise TooManyNeighbours("%d points within the salient radius of point %d" % (c, i))
        m, S = [0, 0, 0], [[0] * 3 for _ in range(3)]
        for j in nb:
            g = [int(math.floor((P[j][a] - P[i][a]) * scale)) for a in range(3)]
            for a in range(3):
                assert abs(g[a]) <= (1 << BITS) + 1
                m[a] += g[a]
                for b in range(3):
                    S[a][b] += g[a] * g[b]
        A = [[0.0] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(3):
                D = c * S[a][b] - m[a] * m[b]
                assert abs(c * S[a][b]) < LIMIT and abs(m[a] * m[b]) < LIMIT and abs(D) < LIMIT
                A[a][b] = float(D) / float(c * c)
        A = _jacobi_scalar(A)
        l1, l2, l3 = sorted((A[0][0], A[1][1], A[2][2]), reverse=True)
        eig.append((l1, l2, l3))
        cs[i] = c
        if c >= min_neighbors and l2 < gamma21 * l1 and l3 < gamma32 * l2 and l3 > 0:
            sal[i] = l3 * unscale
    cn, idx = [0] * n, []
    for i in range(n):
        nb = neighbours(i, non_max_radius)
        cn[i] = len(nb)
        beaten = any(sal[j] > sal[i] or (sal[j] == sal[i] and j < i) for j in nb)
        if sal[i] > 0 and cn[i] >= min_neighbors and not beaten:
            idx.append(i)
    idx = np.array(idx, dtype=np.int32)
    pts = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return {"idx": idx, "xyz": np.ascontiguousarray(pts[idx]), "saliency": np.array(sal, dtype=np.float64), "cnt_salient": np.array(cs, dtype=np.int32),
            "cnt_nms": np.array(cn, dtype=np.int32), "eig": np.array(eig, dtype=np.float64).reshape(-1, 3)}


KEYS = (("idx", np.int32), ("xyz", np.float64), ("saliency", np.float64), ("cnt_salient", np.int32), ("cnt_nms", np.int32))


def same(a, b, keys=KEYS):
    """Byte equality of two results."""
    for key, dt in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


# ---- the cases of tests/test_iss_cpu.py and tests/test_gpu_iss.py
CASES = ("bump", "bump_tight", "sheet", "duplicates", "brick")
_cache = {}


def case(name):
    """-> (points, (salient_radius, non_max_radius, gamma21, gamma32, min_neighbors)); the arrays are shared and read-only"""
    if name in _cache:
        return _cache[name]
    import matchref
    import outlierref
    cl = matchref.e2e_clouds()
    r = cl["radius"]
    if name == "bump":
        out = cl["src"], (r, 0.3 * r, 0.975, 0.975, 5)
    elif name == "bump_tight":   # every way of not being a keypoint occurs
        out = cl["src"], (0.5 * r, 0.25 * r, 0.6, 0.05, 8)
    elif name == "sheet":        # planted points far off a thin sheet: neighbourhoods of one or two points, l3 <= 0
        out = outlierref.sheet_cloud(3000, 7)[0], (0.05, 0.03, 0.975, 0.975, 5)
    elif name == "duplicates":   # every point twice, the copies in another order
        a = cl["src"][:700]
        perm = np.random.Generator(np.random.PCG64(5)).permutation(700)
        out = np.concatenate([a, a[perm]], 0), (r, 0.3 * r, 0.975, 0.975, 5)
    elif name == "brick":        # a shuffled lattice with three spacings: exact saliency ties between distinct points
        lat = knnref.shuffled_lattice(7, 3) * np.array([1.0, 1.25, 1.5])
        out = lat, (2.0, 1.3, 0.975, 0.975, 5)
    else:
        raise KeyError(name)
    p = np.ascontiguousarray(out[0], dtype=np.float64)
    p.setflags(write=False)
    _cache[name] = (p, out[1])
    return _cache[name]


def reference(name):
    """iss() of a case, computed once"""
    key = ("ref", name)
    if key not in _cache:
        p, args = case(name)
        _cache[key] = iss(p, *args)
    return _cache[key]


# ---- the clouds-alone initialisation on keypoints (mvicp.init_from_clouds(keypoints=...)) on the CPU
def chain(xyz, desc, edges, params, mode, tau, H, seeds, edge_sim=0.9, min_count=3, root=0):
    """iss per frame -> the rows init_from_clouds hands to mvicp_coarse_pairs (mode "both": the keypoints of both frames; "src": the
    keypoints of the source against the full destination) -> initref.coarse_edge per edge -> poses_from_pairs over the inlier counts and
    the consensus poses.  desc: the descriptors of the FULL clouds.  -> dict(keypoints [K], edges [E] of coarse_edge results, tree)"""
    import initref
    kp = [iss(x, *params)["idx"] for x in xyz]
    out = []
    for (i, j), seed in zip(edges, seeds):
        dj, xj = (desc[j][kp[j]], xyz[j][kp[j]]) if mode == "both" else (desc[j], xyz[j])
        out.append(initref.coarse_edge(np.ascontiguousarray(desc[i][kp[i]]), np.ascontiguousarray(xyz[i][kp[i]]), np.ascontiguousarray(dj),
                                       np.ascontiguousarray(xj), True, 1.0, H, seed, tau, edge_sim))
    tree = initref.poses_from_pairs(len(xyz), [e[0] for e in edges], [e[1] for e in edges], [e["count"] for e in out],
                                    np.array([e["pose"] for e in out]).reshape(-1, 4, 4), min_count, root)
    return {"keypoints": kp, "edges": out, "tree": tree}
