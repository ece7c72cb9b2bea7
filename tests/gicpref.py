"""Extended-precision reference for the plane-to-plane (Generalized-ICP) objective (mvicp_linearize_gicp, csrc/linearize_gicp.hip) of ONE edge.
Test infrastructure only; numpy only.

The rows are written DIRECTLY from the world-frame quantities, in the canonical right-perturbation coordinates T <- T exp([upsilon, omega]) of
both poses — no hi + lo relative transform, no moments, no closed form of the weight, nothing shared with the kernel's algebra:

    e   = R_s p + t_s - R_d q - t_d,      f = R_d^T e                                   (the residual vector in the dst frame)
    nu  = R_d^T R_s n_p,                  P(n) = n n^T / (n . n) if 2^-1022 <= n . n < inf as computed in fp64, else 0
    S   = 2 I - (1 - eps) (P(n_q) + P(nu)),   W = 2 eps S^-1                             (S inverted by cofactors, as it stands)
    J_f = [ A , -A [p]x , -I , [p~]x ],   A = R_d^T R_s,  p~ = R_d^T (R_s p + t_s - t_d)   (W frozen in the dst frame)
    s   = f^T W f;   loss of the point family (soft-L1 on s):  y = 1 + s / a^2, rho' = 1 / sqrt(y), rho / 2 = s / (sqrt(y) + 1)
    H = sum rho' J_f^T W J_f,   g = sum rho' J_f^T W f,   cost = sum rho / 2

rows / edge_block: np.longdouble, pairwise sums.  centred_blocks: the kernel's formulation (Woodbury form of W, moments about the relative
translation, expanded with R6 and L) in long double.  blocks_fp64: the same rows in plain fp64, every sum accumulated serially — the yardstick of
the GPU sweep.  The smallest eigenvalue of S is 2 eps and S is rounded to 2^-64 of its largest entry, so the long-double W is good to
2^-64 / eps relative: 5e-16 at eps = 1e-4, against a bar that is never below 32 x 2^-52 = 7e-15; and 5e-14 at eps = 1e-6, the smallest the
entry points accept, which only the parallel-normals family of the sweep uses (tests/gicpcases.py): the yardstick's worst piece is about 2e-10
there, so the reference is still far inside the bar, but an error of the kernel below 5e-14 cannot be told from the reference's own.
P(n) is taken with the contract's predicate on the fp64 VALUE of n (has_normal below), whatever type the rows are computed in: a normal whose
n . n overflows or underflows fp64 is a missing normal although its long-double n . n is an ordinary number."""
import numpy as np

import xprec
from xprec import LD, _cross, _ld, _psum, piece_errors, unpack, worst_ratio  # noqa: F401  (re-exported for the tests)


TINY = np.finfo(np.float64).tiny     # 2^-1022, the smallest normal fp64 number


def has_normal(n):
    """(3, N) -> the contract's predicate (include/mvicp.h), taken on the fp64 VALUE of n whatever type it is held in: n . n computed in fp64 is
    at least 2^-1022 and finite.  Below that n . n is subnormal or 0 and no longer says how long n is; a NaN compares false."""
    m = np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        nn = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
        return (nn >= TINY) & (nn < np.inf)


def _proj(n, ftype):
    """(3, N) -> P(n) as (3, 3, N); the zero matrix where has_normal(n) is false"""
    ok = has_normal(n)
    m = np.where(ok, n, ftype(0))
    nn = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
    return m[:, None, :] * m[None, :, :] / np.where(ok, nn, ftype(1))


def _inv3(S):
    """inverse of (3, 3, N) matrices by cofactors, in the arrays' own number type"""
    C = np.empty_like(S)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i, j] = S[i1, j1] * S[i2, j2] - S[i1, j2] * S[i2, j1]
    det = S[0, 0] * C[0, 0] + S[0, 1] * C[0, 1] + S[0, 2] * C[0, 2]
    return np.transpose(C, (1, 0, 2)) / det


def weight(nq, nu, eps, ftype=LD):
    """W = 2 eps (2 I - (1 - eps) (P(n_q) + P(nu)))^-1 for (3, N) normals already in one frame -> (3, 3, N)"""
    eps = ftype(eps)
    S = 2 * np.eye(3, dtype=ftype)[:, :, None] - (1 - eps) * (_proj(nq, ftype) + _proj(nu, ftype))
    return 2 * eps * _inv3(S)


def _rows(p, q, nq, npn, Ps, Pd, a, eps, robust, cast, ftype):
    p, q, nq, npn = cast(p).T.copy(), cast(q).T.copy(), cast(nq).T.copy(), cast(npn).T.copy()
    Ps, Pd = cast(Ps), cast(Pd)
    Rs, ts, Rd, td = Ps[:3, :3], Ps[:3, 3:4], Pd[:3, :3], Pd[:3, 3:4]
    N = p.shape[1]
    e = (Rs @ p + ts) - (Rd @ q + td)
    f = Rd.T @ e
    with np.errstate(invalid="ignore", over="ignore"):         # (a NaN, Inf or huge n_p: has_normal says no, whatever nu comes to)
        W = weight(nq, Rd.T @ (Rs @ npn), eps, ftype)
    A = Rd.T @ Rs
    pt = Rd.T @ ((Rs @ p + ts) - td)
    J = np.zeros((12, 3, N), dtype=ftype)
    for c in range(3):
        ec = np.zeros((3, N), dtype=ftype); ec[c] = 1
        J[c] = A[:, c:c + 1]
        J[3 + c] = -(A @ _cross(p, ec))
        J[6 + c] = -ec
        J[9 + c] = _cross(pt, ec)
    Wf = (W * f[None, :, :]).sum(axis=1)
    s = (f * Wf).sum(axis=0)
    if robust:
        a = ftype(np.float32(a))
        sy = np.sqrt(1 + s / (a * a))
        w = np.maximum(ftype(np.finfo(np.float64).tiny), 1 / sy)
        half_rho = s / (sy + 1)
    else:
        w, half_rho = np.ones(N, dtype=ftype), s / 2
    return f, J, W, w, half_rho


def rows(p, q, nq, npn, Ps, Pd, a, eps, robust):
    """Per correspondence, in long double: f (3, N), J_f (12, 3, N) [ups_s om_s ups_d om_d], W (3, 3, N), rho' (N), rho / 2 (N).
    p, npn: source points / normals (N, 3); q, nq: destination points / normals; Ps, Pd: 4x4; a: the scale; eps: the fp64 epsilon."""
    return _rows(p, q, nq, npn, Ps, Pd, a, eps, robust, _ld, LD)


def residual(p, q, nq, npn, Ps, Pd):
    """f in long double (for the central differences of the CPU test)"""
    return rows(p, q, nq, npn, Ps, Pd, 1.0, 1.0, False)[0]


def _sums(f, J, W, w, half_rho, rsum, ftype):
    """the 91 sums of one chunk: per correspondence the three terms over the residual's components are added first, then `rsum` over the list"""
    WJ = np.zeros_like(J)
    for k in range(3):
        for l in range(3):
            WJ[:, k, :] += W[k, l][None, :] * J[:, l, :]
    Wf = (W * f[None, :, :]).sum(axis=1)
    out = np.zeros(91, dtype=ftype)
    o = 0
    for i in range(12):
        Ji = w[None, :] * J[i]
        out[78 + i] = rsum((Ji * Wf).sum(axis=0))
        for j in range(i, 12):
            out[o] = rsum((Ji * WJ[j]).sum(axis=0)); o += 1
    out[90] = rsum(half_rho)
    return out


def _assemble(tot, dtype):
    H = np.zeros((12, 12), dtype=dtype)
    H[np.triu_indices(12)] = tot[:78]
    H = H + np.triu(H, 1).T
    return H, tot[78:90].copy(), tot[90]


def edge_block(p, q, nq, npn, Ps, Pd, a, eps, robust):
    """-> (H 12x12, g 12, cost) in long double: the direct sums (chunked and pairwise like xprec.edge_block)."""
    p, q, nq, npn = np.asarray(p), np.asarray(q), np.asarray(nq), np.asarray(npn)
    parts = []
    for lo in range(0, len(p), xprec.CHUNK):
        sl = slice(lo, lo + xprec.CHUNK)
        parts.append(_sums(*rows(p[sl], q[sl], nq[sl], npn[sl], Ps, Pd, a, eps, robust), _psum, LD))
    tot = _psum(np.array(parts, dtype=LD).T) if parts else np.zeros(91, dtype=LD)
    return _assemble(tot, LD)


def blocks_fp64(p, q, nq, npn, Ps, Pd, a, eps, robust):
    """-> 91 fp64 values [78 upper H | 12 g | cost]: the same rows in plain fp64 (numpy: every operation rounded on its own), each of the 91
    sums accumulated serially in the order of the list, as a loop over the correspondences would."""
    f64 = lambda x: np.asarray(x, dtype=np.float64)   # noqa: E731
    ssum = lambda x: np.cumsum(x, axis=-1)[..., -1]    # noqa: E731
    if len(p) == 0:
        return np.zeros(91)
    return _sums(*_rows(f64(p), f64(q), f64(nq), f64(npn), f64(Ps), f64(Pd), a, eps, robust, f64, np.float64), ssum, np.float64)


def centred_blocks(p, q, nq, npn, Ps, Pd, a, eps, robust):
    """The formulation of csrc/linearize_gicp.hip in long double: A = R_d^T R_s, t = R_d^T (t_s - t_d), x' = A p, f = x' + t - q, the weight in its
    Woodbury form on the normalised normals, the moments U = sum w M W M^T and v = sum w M W f with M = [I ; [x']x] about the relative
    translation, expanded as the plane family: H_ss = R6^T U R6, H_sd = -R6^T U L^T, H_dd = L U L^T, g = [R6^T v ; -L v].  -> (H, g, cost)"""
    p, q, nq, npn = _ld(p).T.copy(), _ld(q).T.copy(), _ld(nq).T.copy(), _ld(npn).T.copy()
    Ps, Pd = _ld(Ps), _ld(Pd)
    A = Pd[:3, :3].T @ Ps[:3, :3]
    t = Pd[:3, :3].T @ (Ps[:3, 3:4] - Pd[:3, 3:4])
    N = p.shape[1]
    x, nu = A @ p, A @ npn
    f = x + t - q

    def unit(n):
        ok = has_normal(n)
        m = np.where(ok, n, LD(0))
        return m / np.sqrt(np.where(ok, (m * m).sum(axis=0), LD(1))), ok

    (ah, oka), (bh, okb) = unit(nq), unit(nu)
    e = LD(eps); c = 1 - e
    d = (ah * bh).sum(axis=0)
    z = _cross(ah, bh)
    zz = np.where(oka & okb, (z * z).sum(axis=0), LD(1))
    kappa = e * c / (4 * e + c * c * zz)
    outer = lambda u, v: u[:, None, :] * v[None, :, :]   # noqa: E731
    W = e * np.eye(3, dtype=LD)[:, :, None] + kappa * ((1 + e) * (outer(ah, ah) + outer(bh, bh)) + c * d * (outer(ah, bh) + outer(bh, ah)))
    Wf = (W * f[None, :, :]).sum(axis=1)
    s = (f * Wf).sum(axis=0)
    if robust:
        aa = LD(np.float32(a))
        sy = np.sqrt(1 + s / (aa * aa))
        w, half_rho = 1 / sy, s / (sy + 1)
    else:
        w, half_rho = np.ones(N, dtype=LD), s / 2
    M = np.zeros((6, 3, N), dtype=LD)          # rows of M: M[i] . g = u'_i for u' = [g ; x' x g]
    for k in range(3):
        ek = np.zeros((3, N), dtype=LD); ek[k] = 1
        M[k] = ek
        M[3:, k, :] = _cross(x, ek)            # column k of [x']x
    WM = np.zeros_like(M)
    for k in range(3):
        for l in range(3):
            WM[:, k, :] += W[k, l][None, :] * M[:, l, :]
    U = np.zeros((6, 6), dtype=LD); v = np.zeros(6, dtype=LD)
    for i in range(6):
        v[i] = _psum(w * (M[i] * Wf).sum(axis=0))
        for j in range(6):
            U[i, j] = _psum(w * (M[i] * WM[j]).sum(axis=0))
    R6 = np.zeros((6, 6), dtype=LD); R6[:3, :3] = A; R6[3:, 3:] = A
    L = np.eye(6, dtype=LD)
    tt = t[:, 0]
    L[3:, :3] = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]], dtype=LD)
    H = np.zeros((12, 12), dtype=LD)
    H[:6, :6] = R6.T @ U @ R6
    H[:6, 6:] = -R6.T @ U @ L.T
    H[6:, :6] = H[:6, 6:].T
    H[6:, 6:] = L @ U @ L.T
    return H, np.concatenate([R6.T @ v, -L @ v]), _psum(half_rho)


def pack(H, g, cost):
    """(H, g, cost) -> the 91 values [78 upper H | 12 g | cost] (inverse of unpack)"""
    return np.concatenate([np.asarray(H)[np.triu_indices(12)], np.asarray(g), [cost]])
