"""The contracts of mvicp_orient_normals and mvicp_signs_from_agreement (include/mvicp.h) on the CPU.

`orient` states mvicp_orient_normals in numpy: the undirected edges of the self-mode mvicp_knn_search rows (knnref), their weights
d = (N_i0 N_j0 + N_i1 N_j1) + N_i2 N_j2, the order (|d| descending, (min index, max index) ascending) by one lexsort, Kruskal over the
sorted arrays, the labels by a walk from every tree's lowest index, the votes by bincount.  `orient_loop` is the same statement one scalar
operation at a time on Python floats, with its own sort and its own union-find.  Every operation is one fp64 operation of numpy or of a
Python float: rounded on its own, never fused.  `signs` / `signs_loop` state mvicp_signs_from_agreement the same two ways, and
`agreement` is the numpy count of mvicp_normal_agreement for one list."""
import math

import numpy as np

import knnref

ANCHOR, VIEWPOINT, DIRECTION = 0, 1, 2


def check_args(k, radius, mode, ref):
    if not 2 <= k <= 64:
        raise ValueError("needs 2 <= k <= 64")
    if not math.isfinite(radius):
        raise ValueError("radius must be finite (<= 0: no radius)")
    if mode not in (ANCHOR, VIEWPOINT, DIRECTION):
        raise ValueError("mode outside {0, 1, 2}")
    if ref is None and mode == DIRECTION:
        raise ValueError("DIRECTION needs a direction")
    r = np.zeros(3) if ref is None else np.asarray(ref, dtype=np.float64).reshape(3)
    if not np.isfinite(r).all():
        raise ValueError("ref must be finite")
    return r


def graph_edges(rows, n):
    """-> (a, b) int64 arrays, a < b: the undirected edges {i, j}, i != j, with j in row i or i in row j, each once, sorted by (a, b)"""
    k = rows["idx"].shape[1] if n else 0
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = rows["idx"].reshape(-1).astype(np.int64)
    keep = (np.arange(k)[None, :] < rows["cnt"][:, None]).reshape(-1) & (j != i) if n else np.zeros(0, dtype=bool)
    i, j = i[keep], j[keep]
    key = np.unique(np.minimum(i, j) * n + np.maximum(i, j))
    return key // max(n, 1), key % max(n, 1)


def _labels(n, adj):
    """comp and x from the forest's adjacency lists adj[i] = [(j, f)]: a walk from every tree's lowest index, in ascending index"""
    comp, x = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    for s in range(n):
        if comp[s] >= 0:
            continue
        comp[s] = s
        stack = [s]
        while stack:
            u = stack.pop()
            for v, f in adj[u]:
                if comp[v] < 0:
                    comp[v] = s; x[v] = x[u] ^ f
                    stack.append(v)
    return comp, x


def orient(p, N, k=10, radius=0.0, mode=ANCHOR, ref=None, rows=None):
    """-> dict(nrm (n, 3), flip (n,) uint8, comp (n,) int32, components) and, for the tests, forest = the (a, b) pairs of the forest's
    edges in the order Kruskal took them, knn = the rows.  A non-finite weight raises ValueError."""
    r = check_args(k, radius, mode, ref)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(N, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    assert len(N) == n
    if rows is None:
        rows = knnref.knn_search(p, None, k, radius)
    a, b = graph_edges(rows, n)
    with np.errstate(all="ignore"):
        d = (N[a, 0] * N[b, 0] + N[a, 1] * N[b, 1]) + N[a, 2] * N[b, 2]
    if not np.isfinite(d).all():
        raise ValueError("a non-finite dot of two normals")
    w, f = np.abs(d), (d < 0).astype(np.uint8)
    order = np.lexsort((b, a, -w))   # w descending, then a, then b ascending
    par = np.arange(n)

    def find(i):
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i

    adj = [[] for _ in range(n)]
    forest = []
    for e in order:
        u, v = int(a[e]), int(b[e])
        ru, rv = find(u), find(v)
        if ru != rv:
            par[ru] = rv
            adj[u].append((v, int(f[e]))); adj[v].append((u, int(f[e])))
            forest.append((u, v))
    comp, x = _labels(n, adj)
    g = np.zeros(n, dtype=np.uint8)
    if mode != ANCHOR and n:
        v = r[None, :] - p if mode == VIEWPOINT else np.broadcast_to(r, (n, 3))
        s = (N[:, 0] * v[:, 0] + N[:, 1] * v[:, 1]) + N[:, 2] * v[:, 2]
        s = np.where(x != 0, -s, s)
        neg = np.bincount(comp, weights=(s < 0), minlength=n).astype(np.int64)
        pos = np.bincount(comp, weights=(s > 0), minlength=n).astype(np.int64)
        g = (neg > pos).astype(np.uint8)
    flip = x ^ g[comp] if n else x
    nrm = np.where((flip != 0)[:, None], -N, N)
    return {"nrm": np.ascontiguousarray(nrm), "flip": flip.astype(np.uint8), "comp": comp, "components": int((comp == np.arange(n)).sum()),
            "forest": forest, "knn": rows}


def orient_loop(p, N, k=10, radius=0.0, mode=ANCHOR, ref=None, rows=None):
    """The same contract, one scalar operation at a time on Python floats (rows: from knnref.knn_search unless given)."""
    r = [float(v) for v in check_args(k, radius, mode, ref)]
    P = [[float(v) for v in row] for row in np.asarray(p, dtype=np.float64).reshape(-1, 3)]
    M = [[float(v) for v in row] for row in np.asarray(N, dtype=np.float64).reshape(-1, 3)]
    n = len(P)
    if rows is None:
        rows = knnref.knn_search(np.asarray(P).reshape(-1, 3), None, k, radius)
    pairs = set()
    for i in range(n):
        for t in range(int(rows["cnt"][i])):
            j = int(rows["idx"][i][t])
            if j != i:
                pairs.add((min(i, j), max(i, j)))
    edges = []
    for u, v in pairs:
        d = (M[u][0] * M[v][0] + M[u][1] * M[v][1]) + M[u][2] * M[v][2]
        if not math.isfinite(d):
            raise ValueError("a non-finite dot of two normals")
        edges.append((-abs(d), u, v, 1 if d < 0 else 0))
    edges.sort()   # (tuples: -w ascending = w descending, then u, then v; -0.0 == 0.0 compare equal, as the bits of |d| do)
    par = list(range(n))
    px = [0] * n   # parity to the parent

    def find(i):
        x = 0
        while par[i] != i:
            x ^= px[i]
            i = par[i]
        return i, x

    for _, u, v, f in edges:
        (ru, xu), (rv, xv) = find(u), find(v)
        if ru == rv:
            continue
        lo, hi = min(ru, rv), max(ru, rv)   # the lower index stays the root: a root is its tree's lowest index
        par[hi] = lo; px[hi] = xu ^ xv ^ f
    comp, x = np.zeros(n, dtype=np.int32), [0] * n
    for i in range(n):
        comp[i], x[i] = find(i)
    neg, pos = [0] * n, [0] * n
    if mode != ANCHOR:
        for i in range(n):
            v = [r[a] - P[i][a] for a in range(3)] if mode == VIEWPOINT else r
            s = (M[i][0] * v[0] + M[i][1] * v[1]) + M[i][2] * v[2]
            if x[i]:
                s = -s
            if s < 0:
                neg[comp[i]] += 1
            if s > 0:
                pos[comp[i]] += 1
    flip, nrm = np.zeros(n, dtype=np.uint8), np.zeros((n, 3))
    for i in range(n):
        flip[i] = x[i] ^ (1 if neg[comp[i]] > pos[comp[i]] else 0)
        nrm[i] = [-M[i][a] for a in range(3)] if flip[i] else M[i]
    return {"nrm": nrm, "flip": flip, "comp": comp, "components": int(sum(1 for i in range(n) if comp[i] == i)), "knn": rows}


KEYS = (("nrm", np.float64), ("flip", np.uint8), ("comp", np.int32))


def same(a, b):
    """Byte equality of two results (signs of zeros included) and of the number of components."""
    for key, dt in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != dt or y.dtype != dt or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return int(a["components"]) == int(b["components"])


# ---- agreement between clouds

def agreement(Ps, Ns, first, Pd, Nd, second):
    """-> (pos, neg) of one list: a = R_src N_first, b = R_dst N_second with the rows of the 4 x 4 poses, t = (a0 b0 + a1 b1) + a2 b2"""
    x, y = np.asarray(Ns, dtype=np.float64)[first], np.asarray(Nd, dtype=np.float64)[second]
    a = [(Ps[r, 0] * x[:, 0] + Ps[r, 1] * x[:, 1]) + Ps[r, 2] * x[:, 2] for r in range(3)]
    b = [(Pd[r, 0] * y[:, 0] + Pd[r, 1] * y[:, 1]) + Pd[r, 2] * y[:, 2] for r in range(3)]
    t = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    return int((t > 0).sum()), int((t < 0).sum())


def check_sign_args(n_frames, src, dst, pos, neg, min_count):
    if n_frames < 1 or min_count < 0 or not (len(src) == len(dst) == len(pos) == len(neg)):
        raise ValueError("bad arguments")
    for e in range(len(src)):
        if not (0 <= src[e] < n_frames and 0 <= dst[e] < n_frames) or src[e] == dst[e] or pos[e] < 0 or neg[e] < 0:
            raise ValueError("bad edge %d" % e)


def signs(n_frames, src, dst, pos, neg, min_count=0):
    """numpy form -> dict(flip (K,) uint8, component (K,) int32, components)"""
    src, dst, pos, neg = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (src, dst, pos, neg))
    check_sign_args(n_frames, src, dst, pos, neg, min_count)
    usable = np.flatnonzero((pos + neg >= min_count) & (pos != neg))
    order = usable[np.lexsort((usable, -np.abs(pos - neg)[usable]))]
    par = np.arange(n_frames)

    def find(i):
        while par[i] != i:
            i = par[i]
        return i

    adj = [[] for _ in range(n_frames)]
    for e in order:
        ru, rv = find(int(src[e])), find(int(dst[e]))
        if ru != rv:
            par[ru] = rv
            f = int(pos[e] < neg[e])
            adj[src[e]].append((int(dst[e]), f)); adj[dst[e]].append((int(src[e]), f))
    comp, x = _labels(n_frames, adj)
    return {"flip": x, "component": comp, "components": int((comp == np.arange(n_frames)).sum())}


def signs_loop(n_frames, src, dst, pos, neg, min_count=0):
    """The same rule as Prim-free plain Python: repeatedly take the first edge of the order that joins two trees."""
    src, dst, pos, neg = ([int(v) for v in np.asarray(a).reshape(-1)] for a in (src, dst, pos, neg))
    check_sign_args(n_frames, src, dst, pos, neg, min_count)
    todo = sorted((e for e in range(len(src)) if pos[e] + neg[e] >= min_count and pos[e] != neg[e]), key=lambda e: (-abs(pos[e] - neg[e]), e))
    tree = list(range(n_frames))   # the tree's lowest frame, kept flat
    x = [0] * n_frames             # parity to it
    for e in todo:
        ta, tb = tree[src[e]], tree[dst[e]]
        if ta == tb:
            continue
        f = 1 if pos[e] < neg[e] else 0
        keep, gone = min(ta, tb), max(ta, tb)
        # parity of the vanishing tree's anchor to the kept one: along anchor .. its end of e .. the other end of e .. the kept anchor
        shift = x[src[e]] ^ x[dst[e]] ^ f
        for i in range(n_frames):
            if tree[i] == gone:
                tree[i] = keep; x[i] ^= shift
    return {"flip": np.array(x, dtype=np.uint8), "component": np.array(tree, dtype=np.int32), "components": len(set(tree))}


def same_signs(a, b):
    return (np.asarray(a["flip"], dtype=np.uint8).tobytes() == np.asarray(b["flip"], dtype=np.uint8).tobytes() and
            np.asarray(a["component"], dtype=np.int32).tobytes() == np.asarray(b["component"], dtype=np.int32).tobytes() and
            int(a["components"]) == int(b["components"]))
