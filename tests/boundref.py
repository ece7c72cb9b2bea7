"""The contract of mvicp_boundary (include/mvicp.h) in numpy (`boundary`), and the same statement as a plain Python loop over scalar floats
(`boundary_loop`).  Per point: the row of the self-mode neighbour search, the unit normal of the chosen source, the tangent frame of
mvicp_fit_normals (jetref), the unit directions of the row's offsets in that frame, and per direction t the question whether another
direction lies counter-clockwise of it by an angle in (0, theta), theta = acos(cos_gap): a direction without one looks into a gap of at
least theta, and a point with such a direction is a boundary point.  Every operation is one fp64 operation of numpy or of a Python float:
rounded on its own, never fused.  `select` is mvicp_boundary_select, `same` / `same_kept` compare results byte for byte."""
import functools
import math

import numpy as np

import knnref

CHUNK = 512   # points per slab of the (n, k, k) sector arrays


def check_args(max_nn, radius, cos_gap, source=0):
    if source not in (0, 1):
        raise ValueError("source must be 0 or 1")
    if not 3 <= max_nn <= 64:
        raise ValueError("max_nn outside [3, 64]")
    if not math.isfinite(radius):
        raise ValueError("radius must be finite")
    if not (math.isfinite(cos_gap) and -1.0 < cos_gap < 1.0):
        raise ValueError("cos_gap must lie in (-1, 1)")


def _rows(p, max_nn, radius, rows):
    return knnref.knn_search(p, None, max_nn, radius) if rows is None else rows


def boundary(p, nrm, max_nn=30, radius=0.0, cos_gap=-0.5, rows=None):
    """-> dict(flag (n,) uint8, open (n,) int32, valid (n,) int32, used (n,) int32, boundary = the number flagged) and, for the tests,
    knn = the rows."""
    check_args(max_nn, radius, cos_gap)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(nrm, dtype=np.float64).reshape(-1, 3)
    n, k = len(p), max_nn
    assert len(N) == n
    rows = _rows(p, max_nn, radius, rows)
    flag, opn, val = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    used = rows["cnt"].astype(np.int32)
    out = {"flag": flag, "open": opn, "valid": val, "used": used, "boundary": 0, "knn": rows}
    if n == 0:
        return out
    cnt = rows["cnt"].astype(np.int64)
    idx = np.maximum(rows["idx"], 0).astype(np.int64)
    for a0 in range(0, n, CHUNK):
        sl = slice(a0, min(a0 + CHUNK, n))
        m = sl.stop - sl.start
        c, Ns = cnt[sl], N[sl]
        inside = np.arange(k)[None, :] < c[:, None]
        with np.errstate(all="ignore"):
            d = np.where(inside[:, :, None], p[idx[sl]] - p[sl][:, None, :], 0.0)      # (m, k, 3)
            l = np.sqrt((Ns[:, 0] * Ns[:, 0] + Ns[:, 1] * Ns[:, 1]) + Ns[:, 2] * Ns[:, 2])
            decided = (l > 0) & (l < np.inf) & (c >= 3)
            nv = Ns / l[:, None]
            # the tangent frame: w = e_a x n for the axis a of the smallest |n_a| (the first of equals), u = w / |w|, v = n x u
            ab = np.abs(nv)
            a = np.where(ab[:, 1] < ab[:, 0], 1, 0)
            a = np.where(ab[:, 2] < np.where(a == 1, ab[:, 1], ab[:, 0]), 2, a)
            zero = np.zeros(m)
            w = np.where((a == 0)[:, None], np.stack([zero, -nv[:, 2], nv[:, 1]], 1),
                         np.where((a == 1)[:, None], np.stack([nv[:, 2], zero, -nv[:, 0]], 1), np.stack([-nv[:, 1], nv[:, 0], zero], 1)))
            u = w / np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])[:, None]
            v = np.stack([nv[:, 1] * u[:, 2] - nv[:, 2] * u[:, 1], nv[:, 2] * u[:, 0] - nv[:, 0] * u[:, 2], nv[:, 0] * u[:, 1] - nv[:, 1] * u[:, 0]], 1)

            def coord(e):
                return (d[:, :, 0] * e[:, None, 0] + d[:, :, 1] * e[:, None, 1]) + d[:, :, 2] * e[:, None, 2]
            x, y = coord(u), coord(v)
            r = np.sqrt(x * x + y * y)
            valid = inside & (r > 0) & (r < np.inf) & decided[:, None]
            ex, ey = x / r, y / r
            # [i, t, s]: s lies in t's sector
            cross = ex[:, :, None] * ey[:, None, :] - ey[:, :, None] * ex[:, None, :]
            dot = ex[:, :, None] * ex[:, None, :] + ey[:, :, None] * ey[:, None, :]
            hit = ((cross > 0) & (dot > cos_gap) & valid[:, None, :]).any(axis=2)
        o = (valid & ~hit).sum(axis=1)
        opn[sl] = o
        val[sl] = valid.sum(axis=1)
        flag[sl] = o > 0
    out["boundary"] = int(flag.sum())
    return out


def boundary_loop(p, nrm, max_nn=30, radius=0.0, cos_gap=-0.5, rows=None, points=None):
    """The same contract, one scalar operation at a time on Python floats.  points: the indices to decide (None: all; a row does not depend
    on the others, and the rest keep flag / open / valid 0)."""
    check_args(max_nn, radius, cos_gap)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    N = np.ascontiguousarray(nrm, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    rows = _rows(p, max_nn, radius, rows)
    flag, opn, val = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    used = rows["cnt"].astype(np.int32)
    inf = math.inf

    for i in (range(n) if points is None else points):
        c = int(rows["cnt"][i])
        N0, N1, N2 = float(N[i, 0]), float(N[i, 1]), float(N[i, 2])
        sq = (N0 * N0 + N1 * N1) + N2 * N2
        l = math.sqrt(sq) if sq >= 0 else math.nan
        if not (0 < l < inf and c >= 3):
            continue
        n0, n1, n2 = N0 / l, N1 / l, N2 / l
        a = 0
        if abs(n1) < abs(n0):
            a = 1
        if abs(n2) < abs((n0, n1)[a]):
            a = 2
        w = ((0.0, -n2, n1), (n2, 0.0, -n0), (-n1, n0, 0.0))[a]
        lw = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        u0, u1, u2 = w[0] / lw, w[1] / lw, w[2] / lw
        v0, v1, v2 = n1 * u2 - n2 * u1, n2 * u0 - n0 * u2, n0 * u1 - n1 * u0
        dirs = []
        for t in range(c):
            j = int(rows["idx"][i, t])
            d0, d1, d2 = float(p[j, 0]) - float(p[i, 0]), float(p[j, 1]) - float(p[i, 1]), float(p[j, 2]) - float(p[i, 2])
            x = (d0 * u0 + d1 * u1) + d2 * u2
            y = (d0 * v0 + d1 * v1) + d2 * v2
            r = math.sqrt(x * x + y * y)
            if 0 < r < inf:
                dirs.append((x / r, y / r))
        o = 0
        for t, (ext, eyt) in enumerate(dirs):
            hit = False
            for exs, eys in dirs:
                if ext * eys - eyt * exs > 0 and ext * exs + eyt * eys > cos_gap:
                    hit = True
                    break
            o += 0 if hit else 1
        opn[i] = o
        val[i] = len(dirs)
        flag[i] = 1 if o > 0 else 0
    return {"flag": flag, "open": opn, "valid": val, "used": used, "boundary": int(flag.sum()), "knn": rows}


def select(p, nrm, res, boundary=True):
    """mvicp_boundary_select: the flagged points (boundary) or the rest, in ascending original index.  nrm = the FRAME's stored normals
    (None: the frame has none), whatever source the flags were computed from."""
    idx = np.flatnonzero(res["flag"] == (1 if boundary else 0)).astype(np.int32)
    p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
    return {"xyz": np.ascontiguousarray(p[idx]), "nrm": None if nrm is None else np.ascontiguousarray(np.asarray(nrm, dtype=np.float64).reshape(-1, 3)[idx]),
            "idx": idx, "kept": len(idx)}


def _bytes_equal(x, y, dt):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == dt and y.dtype == dt and x.shape == y.shape and x.tobytes() == y.tobytes()


KEYS = (("flag", np.uint8), ("open", np.int32), ("valid", np.int32), ("used", np.int32))


def same(a, b):
    """Byte equality of two results."""
    return all(_bytes_equal(a[k], b[k], dt) for k, dt in KEYS) and int(a["boundary"]) == int(b["boundary"])


def same_kept(a, b):
    """Byte equality of two selections."""
    if int(a["kept"]) != int(b["kept"]) or (a["nrm"] is None) != (b["nrm"] is None):
        return False
    if a["nrm"] is not None and not _bytes_equal(a["nrm"], b["nrm"], np.float64):
        return False
    return _bytes_equal(a["xyz"], b["xyz"], np.float64) and _bytes_equal(a["idx"], b["idx"], np.int32)


def reject_by_mask(first, second, src_mask, dst_mask):
    """mvicp.reject_by_mask in its plainest form: the pairs whose ends are both unflagged, in their order."""
    keep = np.ones(len(first), dtype=bool)
    if src_mask is not None:
        keep &= np.asarray(src_mask)[first] == 0
    if dst_mask is not None:
        keep &= np.asarray(dst_mask)[second] == 0
    return first[keep], second[keep]


# ---- the clouds of the tests
def lattice7():
    """The flat 7 x 7 integer lattice (x major) with normals (0, 0, 1): neighbours exactly 90 degrees apart, distances tie exactly."""
    g = np.arange(7, dtype=np.float64)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    p = np.ascontiguousarray(np.concatenate([xy, np.zeros((49, 1))], 1))
    return p, np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (49, 1)))


# open[i] on lattice7 at cos_gap = 0, as rows of x: computed with `boundary` and `boundary_loop` and pinned here
LATTICE_K5 = np.array([[2, 2, 2, 2, 2, 2, 1],
                       [2, 4, 4, 4, 4, 4, 2],
                       [2, 4, 4, 4, 4, 4, 2],
                       [2, 4, 4, 4, 4, 4, 2],
                       [2, 4, 4, 4, 4, 4, 2],
                       [2, 4, 4, 4, 4, 4, 2],
                       [2, 2, 2, 2, 2, 2, 1]], dtype=np.int32)
LATTICE_K9 = np.array([[2, 2, 2, 2, 2, 1, 2],
                       [1, 0, 0, 0, 0, 0, 2],
                       [2, 0, 0, 0, 0, 0, 2],
                       [2, 0, 0, 0, 0, 0, 2],
                       [2, 0, 0, 0, 0, 0, 2],
                       [2, 0, 0, 0, 0, 0, 1],
                       [2, 1, 2, 2, 2, 2, 2]], dtype=np.int32)


def holed_sheet(side=41, hole=(20.3, 19.6), hole_radius=6.0, seed=5):
    """A jittered side x side sheet (pitch 1, jitter +-0.2 in x and y, z a gentle bump) with a planted circular hole, and the sheet's
    mean normal (0, 0, 1) at every point.  -> (points, normals, distance of every point to the hole's rim, distance to the outline)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.arange(side, dtype=np.float64)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + rng.uniform(-0.2, 0.2, size=(side * side, 2))
    rc = np.sqrt(((xy - np.array(hole)) ** 2).sum(1))
    keep = rc >= hole_radius
    xy, rc = xy[keep], rc[keep]
    z = 0.5 * np.sin(xy[:, 0] / 9.0) * np.cos(xy[:, 1] / 11.0)
    p = np.ascontiguousarray(np.concatenate([xy, z[:, None]], 1))
    to_outline = np.minimum(np.minimum(xy[:, 0], xy[:, 1]), np.minimum(side - 1 - xy[:, 0], side - 1 - xy[:, 1]))
    return p, np.ascontiguousarray(np.tile([0.0, 0.0, 1.0], (len(p), 1))), rc - hole_radius, to_outline


HOLE_MARGIN = 1.5   # spacings: no point farther than this from the hole's rim and from the outline may be flagged (observed: 0.97)


def _unit(v):
    return v / np.sqrt((v * v).sum(1))[:, None]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (points, normals, ((max_nn, radius, cos_gap), ..)): the clouds the CPU and the GPU tests share.  What each is for is asserted
    on the reference in tests/test_boundary_cpu.py::test_the_cases_hold_what_they_are_for."""
    import matchref
    rng = np.random.Generator(np.random.PCG64(77))
    out = {}
    # a flat blob: a Gaussian disc, thin in z, normals near +z of any length in [0.5, 2)
    blob = rng.normal(size=(2000, 3)) * np.array([1.0, 1.0, 0.05])
    bn = _unit(np.array([0.0, 0.0, 1.0]) + 0.1 * rng.normal(size=(2000, 3))) * rng.uniform(0.5, 2.0, size=(2000, 1))
    out["blob"] = (blob, bn, ((3, 0.0, -0.5), (10, 0.0, -0.5), (64, 0.0, -0.5)))
    cl = matchref.e2e_clouds(False)
    out["e2e dst"] = (cl["dst"], cl["dst_nrm"], ((30, 0.0, -0.5), (30, 0.0, 0.0)))
    lp, ln = lattice7()
    perm = rng.permutation(49)
    out["lattice, shuffled"] = (lp[perm], ln[perm], ((5, 0.0, 0.0), (9, 0.0, 0.0)))
    # every point six times: at max_nn <= 6 a row holds copies only, at 30 it reaches other points
    base, bnrm = matchref.bumps(120, 31)
    out["duplicated"] = (np.repeat(base, 6, axis=0), np.repeat(bnrm, 6, axis=0), ((5, 0.0, -0.5), (6, 0.0, -0.5), (30, 0.0, -0.5)))
    t = np.sort(rng.uniform(0.0, 1.0, size=300))
    line = np.stack([1.0 + 2.0 * t, -0.5 + 0.5 * t, 3.0 - t], 1)
    out["collinear"] = (line, np.tile(_unit(np.array([[1.0, 2.0, 3.0]])), (300, 1)), ((8, 0.0, -0.5), (8, 0.0, 0.9)))
    # normals of length 1e-3 and 1e3, zero normals and NaN normals, a quarter each in index order 0, 1, 2, 3 mod 4
    sp, sn = matchref.bumps(800, 32)
    sn = sn.copy()
    sn[0::4] *= 1e-3; sn[1::4] *= 1e3; sn[2::4] = 0.0; sn[3::4, 1] = np.nan
    sn[2] = -0.0
    out["normal lengths"] = (sp, sn, ((16, 0.0, -0.5),))
    mp, mn = matchref.bumps(800, 33)
    out["scale 1e-3 at 1e3"] = (mp * 1e-3 + 1e3, mn, ((16, 0.0, -0.5),))
    # hybrid rows: the radius of about four neighbours, so that rows run from the point alone to full
    hp, hn = matchref.bumps(800, 34)
    out["hybrid rows"] = (hp, hn, ((8, 0.04, -0.5), (8, 0.04, 0.0)))
    for m in (0, 1, 2, 3):
        out["n = %d" % m] = (hp[:m], hn[:m], ((3, 0.0, -0.5),))
    return {k: (np.ascontiguousarray(p), np.ascontiguousarray(N), runs) for k, (p, N, runs) in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name, run):
    """The reference result of run `run` of cases()[name], computed once and shared; nobody writes into it."""
    p, N, runs = cases()[name]
    r = boundary(p, N, *runs[run])
    for key, _ in KEYS:
        r[key].setflags(write=False)
    return r
