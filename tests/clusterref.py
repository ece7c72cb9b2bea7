"""The contract of mvicp_cluster / mvicp_cluster_keep_rule / mvicp_cluster_select (include/mvicp.h) in numpy: slabbed brute-force distances in
the metric's operation order, the strict predicate sqrt(d2) < radius, counts, a frontier search over the core graph and an argmin per border
point.  `cluster_loop` is the same statement as a plain Python loop over scalars with a stack."""
import math

import numpy as np

SLAB = 512


def dist2_slab(p, a):
    """(d0 d0 + d1 d1) + d2 d2 of the rows a .. a + SLAB against all points, every operation rounded on its own (numpy never contracts)."""
    d = p[a:a + SLAB, None, :] - p[None, :, :]
    return (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]


def can_overflow(p):
    """The rule of the overflow error: with a = the largest |coordinate| and t = a + a, (t t + t t) + t t is not finite."""
    if len(p) == 0:
        return False
    with np.errstate(over="ignore"):
        t = np.float64(np.abs(p).max()) * 2.0
        return not np.isfinite((t * t + t * t) + t * t)


def adjacency(p, radius):
    """The n x n boolean matrix of j in N(i)."""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    A = np.zeros((len(p), len(p)), dtype=bool)
    for a in range(0, len(p), SLAB):
        A[a:a + SLAB] = np.sqrt(dist2_slab(p, a)) < radius
    return A


def _stats(n, label, core, size, has_normals):
    C = len(size)
    largest = int(size.max()) if C else 0
    return {"n": n, "clusters": C, "core": int(core.sum()), "border": int(((label >= 0) & (core == 0)).sum()), "noise": int((label < 0).sum()),
            "largest": largest, "largest_label": int(np.argmax(size)) if C else -1, "has_normals": int(has_normals)}   # (argmax: the first = lowest label)


def cluster(p, nrm, radius, min_pts):
    """-> dict(label (n,) int32, core (n,) uint8, size (C,) int32, stats)."""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    if not (math.isfinite(radius) and radius > 0) or not 1 <= min_pts <= 1 << 30:
        raise ValueError("needs a finite radius > 0 and 1 <= min_pts <= 2^30")
    if can_overflow(p):
        raise OverflowError("a neighbour distance can overflow")
    A = adjacency(p, radius)
    core = A.sum(1) >= min_pts
    label = np.full(n, -1, dtype=np.int32)
    C = 0
    for s in np.flatnonzero(core):          # ascending: a cluster is numbered when its smallest core index is met
        if label[s] >= 0:
            continue
        front = np.zeros(n, dtype=bool); front[s] = True
        seen = front.copy()
        while front.any():
            front = A[front].any(0) & core & ~seen
            seen |= front
        label[seen] = C
        C += 1
    # border: the first core point of N(i) in the order (d2, index); argmin returns the first = lowest index among equal values
    for a in range(0, n, SLAB):
        rows = np.flatnonzero(~core[a:a + SLAB])
        if len(rows) == 0:
            continue
        D = np.where(A[a:a + SLAB] & core[None, :], dist2_slab(p, a), np.inf)[rows]
        j = np.argmin(D, axis=1)
        has = np.isfinite(D[np.arange(len(rows)), j])
        label[a + rows[has]] = label[j[has]]
    size = np.bincount(label[label >= 0], minlength=C).astype(np.int32)
    core = core.astype(np.uint8)
    return {"label": label, "core": core, "size": size, "stats": _stats(n, label, core, size, nrm is not None)}


def cluster_loop(p, nrm, radius, min_pts):
    """The same contract, one scalar operation at a time."""
    n = len(p)
    P = [[float(v) for v in row] for row in p]

    def d2(i, j):
        a, b, c = P[i][0] - P[j][0], P[i][1] - P[j][1], P[i][2] - P[j][2]
        return (a * a + b * b) + c * c

    N = [[j for j in range(n) if math.sqrt(d2(i, j)) < radius] for i in range(n)]
    core = [len(N[i]) >= min_pts for i in range(n)]
    label = [-1] * n
    C = 0
    for s in range(n):
        if not core[s] or label[s] >= 0:
            continue
        label[s] = C
        stack = [s]
        while stack:
            i = stack.pop()
            for j in N[i]:
                if core[j] and label[j] < 0:
                    label[j] = C
                    stack.append(j)
        C += 1
    border = {}
    for i in range(n):
        if core[i]:
            continue
        cands = [(d2(i, j), j) for j in N[i] if core[j]]
        if cands:
            border[i] = label[min(cands)[1]]   # tuples: by d2, then by j
    for i, c in border.items():
        label[i] = c
    size = [0] * C
    for c in label:
        if c >= 0:
            size[c] += 1
    label, core, size = np.array(label, dtype=np.int32).reshape(n), np.array(core, dtype=np.uint8).reshape(n), np.array(size, dtype=np.int32).reshape(C)
    return {"label": label, "core": core, "size": size, "stats": _stats(n, label, core, size, nrm is not None)}


def keep_rule(size, min_size, max_clusters):
    """keep[c] = size[c] >= min_size and (max_clusters == 0 or rank(c) < max_clusters), ranks by (size descending, label ascending)."""
    if min_size < 0 or max_clusters < 0:
        raise ValueError("negative argument")
    order = sorted(range(len(size)), key=lambda c: (-int(size[c]), c))
    keep = np.zeros(len(size), dtype=np.uint8)
    for rank, c in enumerate(order):
        keep[c] = int(size[c]) >= min_size and (max_clusters == 0 or rank < max_clusters)
    return keep


def select(p, nrm, res, min_size, max_clusters):
    """The rows of the kept clusters in ascending original index -> dict(xyz, nrm or None, idx int32, label int32, kept)."""
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    keep = keep_rule(res["size"], min_size, max_clusters)
    lab = res["label"]
    on = lab >= 0
    on[on] = keep[lab[on]] != 0
    idx = np.flatnonzero(on).astype(np.int32)
    return {"xyz": p[idx], "nrm": None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float64)[idx], "idx": idx, "label": lab[idx].astype(np.int32),
            "kept": len(idx)}


STAT_KEYS = ("n", "clusters", "core", "border", "noise", "largest", "largest_label", "has_normals")


def _same_arrays(a, b, keys):
    for key, dt in keys:
        if (a[key] is None) != (b[key] is None):
            return False
        if a[key] is None:
            continue
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


def same(a, b):
    """Byte equality of two cluster results, stats included."""
    return _same_arrays(a, b, (("label", np.int32), ("core", np.uint8), ("size", np.int32))) and all(int(a["stats"][k]) == int(b["stats"][k]) for k in STAT_KEYS)


def same_kept(a, b):
    """Byte equality of two selections."""
    return _same_arrays(a, b, (("xyz", np.float64), ("nrm", np.float64), ("idx", np.int32), ("label", np.int32))) and int(a["kept"]) == int(b["kept"])


# ---- the clouds of the tests
def _unit_normals(rng, n):
    nr = rng.normal(size=(n, 3))
    return nr / np.linalg.norm(nr, axis=1, keepdims=True)


BLOBS_RADIUS = 0.02


def blobs_cloud():
    """Three Gaussian blobs of 800 points (sigma 0.03) and 300 uniform points in [-0.3, 0.6]^3, shuffled -> (points, unit normals)."""
    rng = np.random.Generator(np.random.PCG64(7))
    parts = [np.array(c) + rng.normal(0.0, 0.03, size=(800, 3)) for c in ((0.0, 0.0, 0.0), (0.3, 0.0, 0.0), (0.0, 0.35, 0.1))]
    parts.append(rng.uniform(-0.3, 0.6, size=(300, 3)))
    p = np.concatenate(parts, 0)
    p = np.ascontiguousarray(p[rng.permutation(len(p))])
    return p, _unit_normals(rng, len(p))


SHEET_RADIUS, SHEET_MIN_PTS = 0.04, 4


def sheet_clump_cloud():
    """A 3 000-point sheet (xy uniform in [-0.4, 0.6]^2, z noise sigma 2 mm) followed by a 40-point clump (sigma 4 mm) at (0.1, 0.1, 0.08):
    8 cm off the sheet -> (points, unit normals).  The clump is the rows 3000 .. 3039."""
    rng = np.random.Generator(np.random.PCG64(11))
    p = np.empty((3040, 3))
    p[:3000, :2] = rng.uniform(-0.4, 0.6, size=(3000, 2))
    p[:3000, 2] = rng.normal(0.0, 0.002, size=3000)
    p[3000:] = np.array([0.1, 0.1, 0.08]) + rng.normal(0.0, 0.004, size=(40, 3))
    return p, _unit_normals(rng, len(p))


LATTICE_PITCH = 2.0 ** -8


def dyadic_lattice():
    """8 x 8 x 2 points at pitch 2^-8, x fastest: every coordinate, difference, square and sum is exact."""
    return np.array([[x, y, z] for z in range(2) for y in range(8) for x in range(8)], dtype=np.float64) * LATTICE_PITCH


BRIDGE_PITCH = 2.0 ** -6
BRIDGE_RADIUS = float(np.nextafter(2.0 * BRIDGE_PITCH, 1.0))   # just above two pitches: reaches h, sqrt(2) h, sqrt(3) h and 2 h
BRIDGE_MIN_PTS = 16


def bridge_cloud():
    """Two 4 x 4 x 4 lattice blocks (pitch 2^-6, x in 0 .. 3 and 7 .. 10) joined by the three points x = 4, 5, 6 of the line y = z = 1:
    one pitch apart, each with fewer than BRIDGE_MIN_PTS points within BRIDGE_RADIUS.  The middle one, x = 5, is exactly two pitches
    from (3, 1, 1) and from (7, 1, 1), core points of the one and of the other block.  Shuffled -> (points, index of the middle point)."""
    block = [[x, y, z] for x in range(4) for y in range(4) for z in range(4)]
    pts = np.array(block + [[x + 7, y, z] for x, y, z in block] + [[4, 1, 1], [5, 1, 1], [6, 1, 1]], dtype=np.float64) * BRIDGE_PITCH
    rng = np.random.Generator(np.random.PCG64(21))
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), int(np.flatnonzero(perm == 129)[0])


HELIX_STEP = math.sqrt(9.0 + 0.25) * 0.01   # the speed of (cos 3t, sin 3t, t / 2) times the step of t: the arc between two points


def helix_cloud(n=4096, order="index"):
    """(cos 3t, sin 3t, t / 2), t = 0.01 i: a chain whose links are shorter than 1.5 HELIX_STEP and whose second neighbours are farther."""
    t = 0.01 * np.arange(n)
    p = np.column_stack([np.cos(3.0 * t), np.sin(3.0 * t), t / 2.0])
    if order == "reversed":
        p = p[::-1]
    elif order == "shuffled":
        p = p[np.random.Generator(np.random.PCG64(31)).permutation(n)]
    return np.ascontiguousarray(p)


def line_cloud():
    """400 points on a line along x, off the origin, shuffled: the hash grid is one occupied layer thick along two axes."""
    rng = np.random.Generator(np.random.PCG64(9))
    t = np.sort(rng.uniform(0.0, 2.0, size=400))
    p = np.outer(t, [1.0, 0.0, 0.0]) + [0.5, -0.25, 3.0]
    return np.ascontiguousarray(p[rng.permutation(len(p))])
