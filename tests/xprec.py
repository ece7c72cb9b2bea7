"""Extended-precision (np.longdouble, 64-bit significand) reference for the normal equations of ONE edge.  Test infrastructure only.

Restates per correspondence what the functors of include/icp-ceres.h and ceres::SoftLOneLoss compute, in the world frame like they do, and
writes the Jacobian rows DIRECTLY in the canonical right-perturbation coordinates T <- T exp([upsilon, omega]) of both poses (the
coordinates of orclib.Oracle.edge_blocks) — no moment algebra, no relative transform, nothing shared with csrc/linearize.hip:

    p_w = R_s p + t_s,  q_w = R_d q + t_d,  n_w = R_d n,  e = p_w - q_w
    point-to-point   r = e                J_s = [ R_s , -R_s [p]x ]                 J_d = [ -R_d , R_d [q]x ]
    point-to-plane   r = n_w . e          J_s = [ m ; p x m ]^T, m = R_s^T n_w      J_d = [ -n ; n x (q + R_d^T e) ]^T
    loss (robust)    y = 1 + |r|^2 / a^2, rho' = 1 / sqrt(y), rho / 2 = |r|^2 / (sqrt(y) + 1)   (= a^2 (sqrt(y) - 1) without its cancellation)
    H = sum rho' J^T J,  g = sum rho' J^T r,  cost = sum rho / 2   (Ceres corrector for rho'' <= 0: rows and residual times sqrt(rho'))

Inputs are the fp64 values the engine gets (points, normals, 4x4 poses, the float32 scale a), converted exactly; every sum is a pairwise
sum of long doubles (numpy's reduction over a contiguous axis), so the result is good to ~1e-18 of the sum of magnitudes of its terms.
centred_blocks() is the moment formulation of csrc/linearize.hip evaluated in long double: the algebra of the kernel without its rounding."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit significand on this platform: the extended-precision reference is not available"

PIECES = [("H%d%d" % (i, j), i, j) for i in range(4) for j in range(i, 4)]   # the 10 upper 3x3 sub-blocks of H (block order: ups_s, om_s, ups_d, om_d)
FLOOR = 2.0 ** -52


def _ld(a):
    """fp64 input converted exactly; long-double input (the algebra tests) kept as it is"""
    a = np.asarray(a)
    return a if a.dtype == LD else a.astype(np.float64).astype(LD)


def _cross(a, b):
    """rows of a x rows of b; (3, N) arrays"""
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _psum(a):
    """pairwise sum over the last (contiguous) axis"""
    return np.add.reduce(np.ascontiguousarray(a), axis=-1)


def rows(p, q, n, Ps, Pd, a, plane, robust):
    """Per correspondence, in long double: residual (R, N), Jacobian rows J (12, R, N) [ups_s om_s ups_d om_d], corrector sqrt(rho') (N),
    rho / 2 (N).  R = 1 (plane) or 3 (point).  p, q, n: (N, 3) fp64 (n unused for point-to-point); Ps, Pd: 4x4 fp64; a: the scale."""
    p, q = _ld(p).T.copy(), _ld(q).T.copy()
    Ps, Pd = _ld(Ps), _ld(Pd)
    Rs, ts, Rd, td = Ps[:3, :3], Ps[:3, 3:4], Pd[:3, :3], Pd[:3, 3:4]
    N = p.shape[1]
    e = (Rs @ p + ts) - (Rd @ q + td)
    if plane:
        n = _ld(n).T.copy()
        nw = Rd @ n
        r = _psum(np.ascontiguousarray((nw * e).T))[None, :]
        m = Rs.T @ nw
        J = np.concatenate([m, _cross(p, m), -n, _cross(n, q + Rd.T @ e)])[:, None, :]
    else:
        r = e
        J = np.zeros((12, 3, N), dtype=LD)
        for k in range(3):
            for c in range(3):
                ec = np.zeros((3, 1), dtype=LD); ec[c] = 1
                J[c, k] = Rs[k, c]
                J[3 + c, k] = -(Rs[k:k + 1] @ _cross(p, np.broadcast_to(ec, p.shape)))[0]     # (-R_s [p]x)[k, c]
                J[6 + c, k] = -Rd[k, c]
                J[9 + c, k] = (Rd[k:k + 1] @ _cross(q, np.broadcast_to(ec, q.shape)))[0]      # (R_d [q]x)[k, c]
    s = _psum(np.ascontiguousarray((r * r).T))
    if robust:
        a = LD(np.float32(a))
        y = 1 + s / (a * a)
        sy = np.sqrt(y)
        w = np.maximum(LD(np.finfo(np.float64).tiny), 1 / sy)
        corr, half_rho = np.sqrt(w), s / (sy + 1)
    else:
        corr, half_rho = np.ones(N, dtype=LD), s / 2
    return r, J, corr, half_rho


CHUNK = 1 << 16   # correspondences per pass of edge_block (bounds the long-double workspace; partial sums are combined pairwise)


def edge_block(p, q, n, Ps, Pd, a, plane, robust):
    """-> (H 12x12, g 12, cost) in long double: the direct sums of the corrected rows."""
    p, q = np.asarray(p), np.asarray(q)
    n = np.asarray(n) if plane else None
    parts = []
    for lo in range(0, len(p), CHUNK):
        sl = slice(lo, lo + CHUNK)
        r, J, corr, half_rho = rows(p[sl], q[sl], n[sl] if plane else None, Ps, Pd, a, plane, robust)
        Jc = np.ascontiguousarray((J * corr).reshape(12, -1))
        rc = np.ascontiguousarray((r * corr).reshape(-1))
        part = np.zeros(91, dtype=LD)
        o = 0
        for i in range(12):
            part[78 + i] = _psum(Jc[i] * rc)
            for j in range(i, 12):
                part[o] = _psum(Jc[i] * Jc[j]); o += 1
        part[90] = _psum(half_rho)
        parts.append(part)
    tot = _psum(np.array(parts, dtype=LD).T) if parts else np.zeros(91, dtype=LD)
    H = np.zeros((12, 12), dtype=LD)
    H[np.triu_indices(12)] = tot[:78]
    H = H + np.triu(H, 1).T
    return H, tot[78:90].copy(), tot[90]


def centred_blocks(p, q, n, Ps, Pd, a, plane, robust):
    """The formulation of csrc/linearize.hip in long double: moments of u' = [n ; x' x n] (plane) resp. u'_k = [e_k ; x' x e_k] (point) with
    x' = A p about the relative translation t, expanded with R6 = diag(A, A) and L = [[I, 0], [[t]x, I]]:
    H_ss = R6^T S R6, H_sd = -R6^T (S - X) L^T, H_dd = L (S - X - X^T + Y) L^T, g = [R6^T v ; -L v].  -> (H, g, cost)."""
    p, q = _ld(p).T.copy(), _ld(q).T.copy()
    Ps, Pd = _ld(Ps), _ld(Pd)
    A = Pd[:3, :3].T @ Ps[:3, :3]
    t = Pd[:3, :3].T @ (Ps[:3, 3:4] - Pd[:3, 3:4])
    x = A @ p
    N = p.shape[1]
    S, X, Y = (np.zeros((6, 6), dtype=LD) for _ in range(3))
    v = np.zeros(6, dtype=LD)

    def weights(s):
        if not robust:
            return np.ones(N, dtype=LD), s / 2
        aa = LD(np.float32(a))
        sy = np.sqrt(1 + s / (aa * aa))
        return 1 / sy, s / (sy + 1)

    if plane:
        n = _ld(n).T.copy()
        r = _psum(np.ascontiguousarray((n * (x + t - q)).T))
        w, half_rho = weights(r * r)
        u = np.concatenate([n, _cross(x, n)])
        for i in range(6):
            v[i] = _psum(w * r * u[i])
            for j in range(6):
                S[i, j] = _psum(w * u[i] * u[j])
    else:
        r = x + t - q
        w, half_rho = weights(_psum(np.ascontiguousarray((r * r).T)))
        for k in range(3):
            ek = np.zeros((3, N), dtype=LD); ek[k] = 1
            u = np.concatenate([ek, _cross(x, ek)])
            z = np.concatenate([np.zeros((3, N), dtype=LD), _cross(r, ek)])
            for i in range(6):
                v[i] += _psum(w * r[k] * u[i])
                for j in range(6):
                    S[i, j] += _psum(w * u[i] * u[j]); X[i, j] += _psum(w * u[i] * z[j]); Y[i, j] += _psum(w * z[i] * z[j])
    R6 = np.zeros((6, 6), dtype=LD); R6[:3, :3] = A; R6[3:, 3:] = A
    L = np.eye(6, dtype=LD)
    tt = t[:, 0]
    L[3:, :3] = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]], dtype=LD)
    H = np.zeros((12, 12), dtype=LD)
    H[:6, :6] = R6.T @ S @ R6
    H[:6, 6:] = -R6.T @ (S - X) @ L.T
    H[6:, :6] = H[:6, 6:].T
    H[6:, 6:] = L @ (S - X - X.T + Y) @ L.T
    g = np.concatenate([R6.T @ v, -L @ v])
    return H, g, _psum(half_rho)


def unpack(block):
    """91 fp64 values [78 upper H | 12 g | cost] -> (H 12x12 symmetric, g, cost)"""
    b = np.asarray(block, dtype=np.float64)
    H = np.zeros((12, 12)); H[np.triu_indices(12)] = b[:78]
    return H + np.triu(H, 1).T, b[78:90].copy(), float(b[90])


def piece_errors(got, ref):
    """got = (H, g, cost) in fp64, ref = (H, g, cost) in long double.  -> {piece: max|got - ref| / max|ref| within the piece}, for the 10 upper
    3x3 sub-blocks of H, the 4 three-vectors of g and the cost.  A piece whose reference is exactly zero reports 0.0 when got is exactly zero
    and inf otherwise."""
    Hg, gg, cg = got
    Hr, gr, cr = ref
    out = {}

    def one(name, x, xr):
        x, xr = np.atleast_1d(np.asarray(x, dtype=np.float64)).astype(LD), np.atleast_1d(np.asarray(xr, dtype=LD))
        den = np.abs(xr).max()
        if den == 0:
            out[name] = 0.0 if not np.any(x) else np.inf
        else:
            out[name] = float(np.abs(x - xr).max() / den)

    for name, i, j in PIECES:
        one(name, Hg[3 * i:3 * i + 3, 3 * j:3 * j + 3], Hr[3 * i:3 * i + 3, 3 * j:3 * j + 3])
    for i in range(4):
        one("g%d" % i, gg[3 * i:3 * i + 3], gr[3 * i:3 * i + 3])
    one("cost", cg, cr)
    return out


def worst_ratio(err_got, err_orc):
    """-> (largest err_got / max(err_orc, 2^-52) over the pieces, its piece).  A piece whose reference is exactly zero and which got misses
    gives inf whatever the oracle did there."""
    worst, where = -1.0, None
    for k, eg in err_got.items():
        ratio = np.inf if np.isinf(eg) else eg / max(err_orc[k], FLOOR)
        if ratio > worst:
            worst, where = ratio, k
    return worst, where
