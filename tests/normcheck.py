"""Accuracy check of PCA normals by their Rayleigh residual, against the covariance of the SAME k-NN sets in long double.  Test infrastructure.

For every point, C = sum (x - mean)(x - mean)^T over its returned neighbours (two-pass, long double, rounded to fp64) and (lambda, V) =
numpy.linalg.eigh(C), ascending.  A normal n is judged by
    | |n| - 1 | <= 1e-15,   n_z <= 0,
    n^T C n - lambda_0 <= bar lambda_2                                   (every point, degenerate sets included),
    angle(n, V[:, 0]) <= bar lambda_2 / (lambda_1 - lambda_0)           where lambda_1 - lambda_0 > 1e-6 lambda_2,
with bar = 32 x the same figure of numpy's own fp64 route on the same sets (two-pass fp64 covariance, then eigh), floored at 2^-52."""
import numpy as np

LD = np.longdouble
MARGIN = 32.0
FLOOR = 2.0 ** -52


def _angle(a, b):
    """angle between the lines spanned by rows of a and b (accurate at small angles: atan2 of |a x b| and |a . b|)"""
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.sum(a * b, axis=1)))


def figures(pts, knn, nrm):
    """-> dict of per-point arrays: res / ang of the given normals and res_np / ang_np of numpy's fp64 route (residuals over lambda_2, angles
    times (lambda_1 - lambda_0) / lambda_2; 0 where lambda_2 == 0), gap_ok, norm_err, lam"""
    pts = np.asarray(pts, dtype=np.float64)
    valid = knn >= 0
    nb = pts[np.where(valid, knn, 0)]                                   # (n, k, 3)
    wl = valid[:, :, None].astype(LD)
    cnt = valid.sum(axis=1)[:, None].astype(LD)
    xl = nb.astype(LD)
    dl = (xl - (xl * wl).sum(axis=1, keepdims=True) / cnt[:, :, None]) * wl
    C_ld = np.einsum("nki,nkj->nij", dl, dl)
    C = C_ld.astype(np.float64)
    lam, V = np.linalg.eigh(C)
    w64 = valid[:, :, None].astype(np.float64)
    d64 = (nb - (nb * w64).sum(axis=1, keepdims=True) / valid.sum(axis=1)[:, None, None]) * w64
    _, V64 = np.linalg.eigh(np.einsum("nki,nkj->nij", d64, d64))
    l2 = lam[:, 2]
    safe = np.where(l2 > 0, l2, 1.0)
    gap = lam[:, 1] - lam[:, 0]

    def rayleigh(n):
        n = n.astype(LD)
        r = np.einsum("ni,nij,nj->n", n, C_ld, n) - lam[:, 0].astype(LD)
        return np.where(l2 > 0, r.astype(np.float64) / safe, 0.0)

    def angle(n):
        return np.where(l2 > 0, _angle(n, V[:, :, 0]) * gap / safe, 0.0)

    nl = np.asarray(nrm, dtype=np.float64).astype(LD)
    return {"res": rayleigh(np.asarray(nrm, dtype=np.float64)), "res_np": rayleigh(V64[:, :, 0]), "ang": angle(nrm), "ang_np": angle(V64[:, :, 0]),
            "gap_ok": (l2 > 0) & (gap > 1e-6 * l2), "norm_err": np.abs(np.sqrt((nl * nl).sum(axis=1)) - 1).astype(np.float64), "lam": lam}


def check(pts, knn, nrm, label=""):
    """asserts the four criteria for every point; -> (worst residual ratio, worst angle ratio) against numpy's floored figures"""
    nrm = np.asarray(nrm, dtype=np.float64)
    assert np.all(np.isfinite(nrm)), label
    f = figures(pts, knn, nrm)
    assert f["norm_err"].max() <= 1e-15, (label, f["norm_err"].max())
    assert np.all(nrm[:, 2] <= 0), label
    r_res = f["res"] / np.maximum(f["res_np"], FLOOR)
    r_ang = np.where(f["gap_ok"], f["ang"] / np.maximum(f["ang_np"], FLOOR), 0.0)
    worst = (float(r_res.max()), float(r_ang.max()))
    print("NORMALS %-40s n=%5d  Rayleigh residual / lambda_2: kernel %.1e numpy %.1e ratio %.2f | angle x gap / lambda_2 (%d pts): kernel %.1e numpy %.1e ratio %.2f" % (
        label, len(nrm), f["res"].max(), f["res_np"].max(), worst[0], int(f["gap_ok"].sum()), np.where(f["gap_ok"], f["ang"], 0).max(),
        np.where(f["gap_ok"], f["ang_np"], 0).max(), worst[1]))
    assert worst[0] <= MARGIN, (label, "Rayleigh residual", worst[0], int(r_res.argmax()))
    assert worst[1] <= MARGIN, (label, "angle", worst[1], int(r_ang.argmax()))
    return worst
