"""The numpy statement of the voxel-grid contract (include/mvicp.h, mvicp_voxel_grid): test infrastructure only.

Everything is elementwise numpy on float64 arrays, which evaluates one rounded operation at a time (no fused multiply-add), with the
IEEE division np.floor(W / h); the per-voxel sums are np.add.at into zero arrays, which numpy applies unbuffered in index order, i.e.
s = +0.0; s = s + w in ascending seq.  tests/test_voxel_cpu.py checks this module against a plain Python loop byte for byte."""
import math

import numpy as np


def world(pts_list, nor_list, frames=None, poses=None):
    """The input sequence in world coordinates -> (W (N,3), M (N,3) or None, has_normals)."""
    K = len(pts_list)
    sel = list(range(K)) if frames is None else [int(f) for f in frames]
    assert len(set(sel)) == len(sel) and all(0 <= f < K for f in sel)
    W, M, has = [], [], True
    for f in sel:
        p = np.asarray(pts_list[f], dtype=np.float64).reshape(-1, 3)
        if len(p) == 0:
            continue
        n = None if nor_list is None or nor_list[f] is None else np.asarray(nor_list[f], dtype=np.float64).reshape(-1, 3)
        if n is None:
            has = False
        if poses is None:
            w, m = p, n
        else:
            R = np.asarray(poses[f], dtype=np.float64)[:3, :3]
            t = np.asarray(poses[f], dtype=np.float64)[:3, 3]
            w = np.stack([((R[c, 0] * p[:, 0] + R[c, 1] * p[:, 1]) + R[c, 2] * p[:, 2]) + t[c] for c in range(3)], axis=1)
            m = None if n is None else np.stack([(R[c, 0] * n[:, 0] + R[c, 1] * n[:, 1]) + R[c, 2] * n[:, 2] for c in range(3)], axis=1)
        W.append(w)
        if m is not None:
            M.append(m)
    if not W:
        return np.zeros((0, 3)), np.zeros((0, 3)), True
    return np.concatenate(W), (np.concatenate(M) if has else None), has


def cells(W, h, reciprocal=False):
    """floor(W / h) as int64; reciprocal=True is the WRONG rule floor(W * (1 / h)) (used only to show that a case tells them apart)."""
    with np.errstate(all="ignore"):
        Q = W * (1.0 / h) if reciprocal else W / h
    if not (np.isfinite(Q).all() and (np.abs(Q) < 2.0 ** 31).all()):
        raise ValueError("quotient not finite or >= 2^31")
    return np.floor(Q).astype(np.int64)


def voxel_grid(pts_list, nor_list, voxel, frames=None, poses=None):
    """-> dict(xyz (m,3), nrm (m,3) or None, cnt (m,) int32), rows in ascending key.  ValueError where the library reports MVICP_ERR_ARG."""
    h = float(voxel)
    if not (math.isfinite(h) and h > 0.0):
        raise ValueError("voxel must be finite and > 0")
    W, M, has = world(pts_list, nor_list, frames, poses)
    if len(W) == 0:
        return {"xyz": np.zeros((0, 3)), "nrm": np.zeros((0, 3)), "cnt": np.zeros(0, dtype=np.int32)}
    Cc = cells(W, h)
    cmin = Cc.min(axis=0)
    d = Cc.max(axis=0) - cmin + 1
    if int(d[0]) * int(d[1]) * int(d[2]) >= 2 ** 62:
        raise ValueError("voxel too small for the extent")
    key = ((Cc[:, 2] - cmin[2]) * d[1] + (Cc[:, 1] - cmin[1])) * d[0] + (Cc[:, 0] - cmin[0])
    _, inv = np.unique(key, return_inverse=True)          # rows in ascending key
    inv = inv.reshape(-1)
    m = int(inv.max()) + 1
    cnt = np.bincount(inv, minlength=m).astype(np.int32)
    S = np.zeros((3, m))
    for c in range(3):
        np.add.at(S[c], inv, W[:, c])                     # in index order = ascending seq
    xyz = np.ascontiguousarray((S / cnt.astype(np.float64)).T)
    nrm = None
    if has:
        T = np.zeros((3, m))
        for c in range(3):
            np.add.at(T[c], inv, M[:, c])
        with np.errstate(all="ignore"):
            ln = np.sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2])
            ok = np.isfinite(ln) & (ln > 0.0)
            nrm = np.ascontiguousarray(np.where(ok, T / ln, 0.0).T)
    return {"xyz": xyz, "nrm": nrm, "cnt": cnt}


def voxel_grid_loop(pts_list, nor_list, voxel, frames=None, poses=None):
    """The same definition as a plain Python loop over Python floats (IEEE doubles, one rounded operation at a time)."""
    K = len(pts_list)
    sel = list(range(K)) if frames is None else list(frames)
    h = float(voxel)
    seq, has = [], True
    for f in sel:
        p = np.asarray(pts_list[f], dtype=np.float64).reshape(-1, 3)
        n = None if nor_list is None or nor_list[f] is None else np.asarray(nor_list[f], dtype=np.float64).reshape(-1, 3)
        if len(p) and n is None:
            has = False
        for i in range(len(p)):
            x = [float(v) for v in p[i]]
            y = None if n is None else [float(v) for v in n[i]]
            if poses is not None:
                R = [[float(poses[f][a][b]) for b in range(3)] for a in range(3)]
                t = [float(poses[f][a][3]) for a in range(3)]
                x = [((R[c][0] * x[0] + R[c][1] * x[1]) + R[c][2] * x[2]) + t[c] for c in range(3)]
                if y is not None:
                    y = [(R[c][0] * y[0] + R[c][1] * y[1]) + R[c][2] * y[2] for c in range(3)]
            seq.append((x, y))
    if not seq:
        return {"xyz": np.zeros((0, 3)), "nrm": np.zeros((0, 3)), "cnt": np.zeros(0, dtype=np.int32)}
    cell = [[math.floor(w[a] / h) for a in range(3)] for w, _ in seq]
    cmin = [min(c[a] for c in cell) for a in range(3)]
    d = [max(c[a] for c in cell) - cmin[a] + 1 for a in range(3)]
    runs = {}
    for s, c in enumerate(cell):
        runs.setdefault(((c[2] - cmin[2]) * d[1] + (c[1] - cmin[1])) * d[0] + (c[0] - cmin[0]), []).append(s)
    xyz, nrm, cnt = [], [], []
    for key in sorted(runs):
        s3, t3 = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for s in runs[key]:
            for a in range(3):
                s3[a] = s3[a] + seq[s][0][a]
                if has:
                    t3[a] = t3[a] + seq[s][1][a]
        k = len(runs[key])
        cnt.append(k)
        xyz.append([s3[a] / float(k) for a in range(3)])
        if has:
            q = (t3[0] * t3[0] + t3[1] * t3[1]) + t3[2] * t3[2]
            ln = math.sqrt(q) if q >= 0.0 and math.isfinite(q) else math.nan
            nrm.append([t3[a] / ln for a in range(3)] if math.isfinite(ln) and ln > 0.0 else [0.0, 0.0, 0.0])
    return {"xyz": np.array(xyz, dtype=np.float64).reshape(-1, 3), "nrm": np.array(nrm, dtype=np.float64).reshape(-1, 3) if has else None,
            "cnt": np.array(cnt, dtype=np.int32)}


def same(a, b):
    """Two results equal byte for byte (row order included)."""
    if (a["nrm"] is None) != (b["nrm"] is None):
        return False
    for k in ("xyz", "nrm", "cnt"):
        if a[k] is None:
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return False
    return True


# ---- shared cases ------------------------------------------------------------------------------------------------------------------

LATTICE_H = 0.005


def lattice_case():
    """Points ON cell faces: x = k h for k = -2000 .. 1999 (h = 0.005; for 303 of them floor((k h) / h) != k, and the quotient, not k, is the
    contract), y = +0.0 / -0.0 alternating, z on a small signed lattice; then the first 100 points once more with the opposite normal,
    so that those voxels' normal sums cancel to zero (-> a (0,0,0) normal row).  -> (pts (4100,3), nor (4100,3), h)."""
    h = LATTICE_H
    k = np.arange(-2000, 2000)
    x = k * h
    y = np.where(k % 2 == 0, 0.0, -0.0)
    z = ((k % 7) - 3) * h
    pts = np.stack([x, y, z], axis=1)
    rng = np.random.Generator(np.random.PCG64(77))
    nor = rng.normal(size=(len(k), 3))
    nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    pts = np.concatenate([pts, pts[:100]])
    nor = np.concatenate([nor, -nor[:100]])
    return np.ascontiguousarray(pts), np.ascontiguousarray(nor), h


def small_case():
    """200 points for the Python-loop comparison: 149 random ones in a box that straddles the origin, 50 on the faces k h (k = -25 .. 24, with
    -0.0 among the coordinates), and one far away (a voxel with one point).  -> (pts, nor, h)."""
    h = 0.05
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.uniform(-0.2, 0.3, size=(149, 3))
    k = np.arange(-25, 25)
    b = np.stack([k * h, np.where(k % 2 == 0, -0.0, 0.0), (k % 3 - 1) * h], axis=1)
    c = np.array([[3.0, -2.0, 1.0]])
    pts = np.concatenate([a, b, c])
    nor = rng.normal(size=(200, 3))
    nor /= np.linalg.norm(nor, axis=1, keepdims=True)
    return np.ascontiguousarray(pts), np.ascontiguousarray(nor), h
