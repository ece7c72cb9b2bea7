"""Extended-precision reference for the SYMMETRIC point-to-plane objective (MVICP_METRIC_SYMMETRIC, csrc/linearize_sym.hip) of ONE edge.
Test infrastructure only; numpy only.

The rows are written DIRECTLY in the world frame, in the canonical right-perturbation coordinates T <- T exp([upsilon, omega]) of both
poses — no relative transform, no moments, nothing shared with the kernel's algebra:

    e   = R_s p + t_s - R_d q - t_d
    m_w = (R_d n_q + R_s n_p) / 2
    r   = m_w . e
    J_s = [ R_s^T m_w ;  p x R_s^T m_w + (n_p x R_s^T e) / 2 ]
    J_d = [ -R_d^T m_w ; -q x R_d^T m_w + (n_q x R_d^T e) / 2 ]
    loss and sums: those of xprec.rows / xprec.edge_block (plane family)

rows / edge_block: np.longdouble, pairwise sums.  centred_blocks: the kernel's formulation (moments of u' about the relative translation,
expanded with R6 and L) in long double.  blocks_fp64: the same direct rows in plain fp64, every sum accumulated serially — the yardstick
of the GPU sweep, in the part orclib.Oracle.edge_blocks plays for the other two objectives."""
import numpy as np

import xprec
from xprec import LD, _cross, _ld, _psum, piece_errors, unpack, worst_ratio  # noqa: F401  (re-exported for the tests)


def _rows(p, q, nq, npn, Ps, Pd, a, robust, cast, rowsum, ftype):
    """the direct world-frame rows in the number type `cast` produces; (3, N) arrays inside"""
    p, q, nq, npn = cast(p).T.copy(), cast(q).T.copy(), cast(nq).T.copy(), cast(npn).T.copy()
    Ps, Pd = cast(Ps), cast(Pd)
    Rs, ts, Rd, td = Ps[:3, :3], Ps[:3, 3:4], Pd[:3, :3], Pd[:3, 3:4]
    N = p.shape[1]
    e = (Rs @ p + ts) - (Rd @ q + td)
    mw = (Rd @ nq + Rs @ npn) / 2
    r = rowsum(np.ascontiguousarray((mw * e).T))
    ms, md = Rs.T @ mw, Rd.T @ mw
    es, ed = Rs.T @ e, Rd.T @ e
    J = np.concatenate([ms, _cross(p, ms) + _cross(npn, es) / 2, -md, -_cross(q, md) + _cross(nq, ed) / 2])
    s = r * r
    if robust:
        a = ftype(np.float32(a))
        sy = np.sqrt(1 + s / (a * a))
        w = np.maximum(ftype(np.finfo(np.float64).tiny), 1 / sy)
        corr, half_rho = np.sqrt(w), s / (sy + 1)
    else:
        corr, half_rho = np.ones(N, dtype=ftype), s / 2
    return r, J, corr, half_rho


def rows(p, q, nq, npn, Ps, Pd, a, robust):
    """Per correspondence, in long double: residual (N), Jacobian rows J (12, N) [ups_s om_s ups_d om_d], corrector sqrt(rho') (N), rho / 2 (N).
    p, npn: source points / normals (N, 3); q, nq: destination points / normals; Ps, Pd: 4x4; a: the scale."""
    return _rows(p, q, nq, npn, Ps, Pd, a, robust, _ld, _psum, LD)


def residual(p, q, nq, npn, Ps, Pd):
    """the plain residual m_w . e in long double (for the central differences of the CPU test)"""
    return rows(p, q, nq, npn, Ps, Pd, 1.0, False)[0]


def _assemble(tot, dtype):
    H = np.zeros((12, 12), dtype=dtype)
    H[np.triu_indices(12)] = tot[:78]
    H = H + np.triu(H, 1).T
    return H, tot[78:90].copy(), tot[90]


def edge_block(p, q, nq, npn, Ps, Pd, a, robust):
    """-> (H 12x12, g 12, cost) in long double: the direct sums of the corrected rows (chunked and pairwise like xprec.edge_block)."""
    p, q, nq, npn = np.asarray(p), np.asarray(q), np.asarray(nq), np.asarray(npn)
    parts = []
    for lo in range(0, len(p), xprec.CHUNK):
        sl = slice(lo, lo + xprec.CHUNK)
        r, J, corr, half_rho = rows(p[sl], q[sl], nq[sl], npn[sl], Ps, Pd, a, robust)
        Jc = np.ascontiguousarray(J * corr)
        rc = np.ascontiguousarray(r * corr)
        part = np.zeros(91, dtype=LD)
        o = 0
        for i in range(12):
            part[78 + i] = _psum(Jc[i] * rc)
            for j in range(i, 12):
                part[o] = _psum(Jc[i] * Jc[j]); o += 1
        part[90] = _psum(half_rho)
        parts.append(part)
    tot = _psum(np.array(parts, dtype=LD).T) if parts else np.zeros(91, dtype=LD)
    return _assemble(tot, LD)


def blocks_fp64(p, q, nq, npn, Ps, Pd, a, robust):
    """-> 91 fp64 values [78 upper H | 12 g | cost]: the direct world-frame rows in plain fp64 (numpy: every operation rounded on its own), each of
    the 91 sums accumulated serially in the order of the list, as a loop over the correspondences would."""
    f = lambda x: np.asarray(x, dtype=np.float64)   # noqa: E731
    ssum = lambda x: np.cumsum(x, axis=-1)[..., -1] if x.shape[-1] else np.zeros(x.shape[:-1])   # noqa: E731
    out = np.zeros(91)
    if len(p) == 0:
        return out
    r, J, corr, half_rho = _rows(f(p), f(q), f(nq), f(npn), f(Ps), f(Pd), a, robust, f, ssum, np.float64)
    Jc, rc = J * corr, r * corr
    o = 0
    for i in range(12):
        out[78 + i] = ssum(Jc[i] * rc)
        for j in range(i, 12):
            out[o] = ssum(Jc[i] * Jc[j]); o += 1
    out[90] = ssum(half_rho)
    return out


def centred_blocks(p, q, nq, npn, Ps, Pd, a, robust, inv=None, ftype=LD):
    """The formulation of csrc/linearize_sym.hip in long double: with A = R_d^T R_s, t = R_d^T (t_s - t_d), x' = A p, nu = A n_p,
    m = (n_q + nu) / 2, r = m . (x' + t - q), moments of u' = [m ; (x' x n_q + (q - t) x nu) / 2], expanded as the plane family:
    H_ss = R6^T U R6, H_sd = -R6^T U L^T, H_dd = L U L^T, g = [R6^T v ; -L v].  -> (H, g, cost)
    inv: the 3x3 matrix to use in the place of R_d^-1 (default R_d^T; for a destination matrix that is no rotation the library substitutes the
    transpose too, so the default IS what it evaluates there).  ftype=np.float64: the same formulation in plain fp64 with every sum accumulated
    serially — the yardstick where the direct world-frame rows mean nothing (a destination that is no rotation)."""
    if ftype is LD:
        cast, rsum = _ld, _psum
    else:
        cast = lambda x: np.asarray(x, dtype=np.float64)   # noqa: E731
        rsum = lambda x: np.cumsum(x, axis=-1)[..., -1]     # noqa: E731
    p, q, nq, npn = cast(p).T.copy(), cast(q).T.copy(), cast(nq).T.copy(), cast(npn).T.copy()
    Ps, Pd = cast(Ps), cast(Pd)
    Ri = Pd[:3, :3].T if inv is None else cast(inv)
    A = Ri @ Ps[:3, :3]
    t = Ri @ (Ps[:3, 3:4] - Pd[:3, 3:4])
    x, nu = A @ p, A @ npn
    m = (nq + nu) / 2
    r = rsum(np.ascontiguousarray((m * (x + t - q)).T))
    s = r * r
    if robust:
        aa = ftype(np.float32(a))
        sy = np.sqrt(1 + s / (aa * aa))
        w, half_rho = 1 / sy, s / (sy + 1)
    else:
        w, half_rho = np.ones(p.shape[1], dtype=ftype), s / 2
    u = np.concatenate([m, (_cross(x, nq) + _cross(q - t, nu)) / 2])
    U = np.zeros((6, 6), dtype=ftype); v = np.zeros(6, dtype=ftype)
    for i in range(6):
        v[i] = rsum(w * r * u[i])
        for j in range(6):
            U[i, j] = rsum(w * u[i] * u[j])
    R6 = np.zeros((6, 6), dtype=ftype); R6[:3, :3] = A; R6[3:, 3:] = A
    L = np.eye(6, dtype=ftype)
    tt = t[:, 0]
    L[3:, :3] = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]], dtype=ftype)
    H = np.zeros((12, 12), dtype=ftype)
    H[:6, :6] = R6.T @ U @ R6
    H[:6, 6:] = -R6.T @ U @ L.T
    H[6:, :6] = H[:6, 6:].T
    H[6:, 6:] = L @ U @ L.T
    return H, np.concatenate([R6.T @ v, -L @ v]), rsum(half_rho)


def pack(H, g, cost):
    """(H, g, cost) -> the 91 values [78 upper H | 12 g | cost] (inverse of unpack)"""
    return np.concatenate([np.asarray(H)[np.triu_indices(12)], np.asarray(g), [cost]])


# ---- the behaviour claim: a small host registration over either objective (tests/test_sym_cpu.py; its GPU twin is in test_gpu_sym_api.py)
def nn_cutoff(src, Ps, dst, Pd, cutoff):
    """brute-force 1-NN of every source point (moved into the dst frame) with the library's cutoff rule: keep dist < cutoff, scale =
    float32(1.5 x upper median of the kept distances).  -> (first, second, a)"""
    Rel = np.linalg.inv(Pd) @ Ps
    x = src @ Rel[:3, :3].T + Rel[:3, 3]
    d2 = ((x[:, None, :] - dst[None, :, :]) ** 2).sum(-1)
    j = np.argmin(d2, axis=1)
    d = np.sqrt(d2[np.arange(len(src)), j])
    keep = d < float(np.float32(cutoff))
    first, second = np.nonzero(keep)[0].astype(np.int32), j[keep].astype(np.int32)
    kept = np.sort(d[keep])
    a = np.float32(1.5 * kept[len(kept) // 2]) if len(kept) else np.float32(0)
    return first, second, a


def start_pose(truth, spacing, angle_deg=3.0):
    """the truth perturbed by angle_deg about a fixed axis and by one spacing along another"""
    from mvicp import synth
    ax = np.array([1.0, 2.0, -1.5]); ax /= np.linalg.norm(ax)
    tv = np.array([-2.0, 1.0, 2.0]); tv /= np.linalg.norm(tv)
    P = truth.copy()
    P[:3, :3] = truth[:3, :3] @ synth.so3_exp(ax * np.radians(angle_deg))
    P[:3, 3] = truth[:3, 3] + spacing * tv
    return P


def distance_to_truth(P, truth, src, spacing):
    """-> (rotation error in degrees, largest displacement of a source point from its true place in spacings)"""
    from mvicp import synth
    _, ang = synth.pose_diff(P, truth)
    a = src @ P[:3, :3].T + P[:3, 3]
    b = src @ truth[:3, :3].T + truth[:3, 3]
    return float(np.degrees(ang)), float(np.sqrt(((a - b) ** 2).sum(1)).max() / spacing)
