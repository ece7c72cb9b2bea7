"""CPU (-m "not gpu"): the extended-precision reference of tests/xprec.py is pinned against the fp64 oracle, the centred moment algebra of
csrc/linearize.hip is proved in long double, and the oracle's own error on every case of the conditioning sweep
(tests/test_gpu_lin_accuracy.py) is checked to be what rounding analysis predicts, so that "32 x the oracle's error" is a real bar."""
import numpy as np
import pytest

import lincases
import xprec
from mvicp import synth

EPS = 2.0 ** -52
FLAGS = [(1, 1), (1, 0), (0, 1), (0, 0)]   # (point_to_plane, robust)


def test_long_double_has_a_64_bit_significand():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("plane,robust", FLAGS)
def test_extended_reference_agrees_with_the_oracle_on_a_synthetic_problem(orc, plane, robust):
    """synth.make_problem(3, 3000), the lists of one search: orc.edge_blocks (fp64 Jets) against xprec.edge_block (direct long-double rows), piece
    by piece.  Bound: a serial fp64 sum of N terms, each with ~32 roundings of its own, is good to (N + 32) eps of the sum of magnitudes; H's
    diagonal pieces and the cost are sums of one sign, so that is their relative error: 7e-13 at N ~ 3000.  The other pieces cancel and g also
    carries the rounding of the O(1) world coordinates against 1e-2 residuals: they get the suite's 1e-10.
    Observed: H <= 4e-14, cost <= 3e-15, g <= 2e-12."""
    pb = synth.make_problem(3, 3000)
    worst = {"Hdiag": 0.0, "Hoff": 0.0, "g": 0.0, "cost": 0.0}
    for e, (s, d) in enumerate(zip(pb["src"], pb["dst"])):
        f, sec, dist, w, _, _ = orc.correspond_edge(pb["pts"][s], pb["init"][s], pb["pts"][d], pb["init"][d], 0.05)
        assert len(f) > 2000
        want = orc.edge_blocks(pb["pts"], pb["nor"], [s], [d], [(f, sec)], [w], pb["init"], plane, robust)[0]
        ref = xprec.edge_block(pb["pts"][s][f], pb["pts"][d][sec], pb["nor"][d][sec], pb["init"][s], pb["init"][d], w, plane, robust)
        err = xprec.piece_errors(xprec.unpack(want), ref)
        for k, v in err.items():
            kind = "cost" if k == "cost" else "g" if k[0] == "g" else "Hdiag" if k[1] == k[2] else "Hoff"
            worst[kind] = max(worst[kind], v)
    print("oracle vs extended reference (plane=%d robust=%d): %s" % (plane, robust, {k: "%.1e" % v for k, v in worst.items()}))
    bound = (len(f) + 32) * EPS
    assert worst["Hdiag"] <= bound and worst["cost"] <= bound, worst
    assert worst["Hoff"] <= 1e-10 and worst["g"] <= 1e-10, worst


def _ld_pose(rng, tnorm):
    """a pose whose rotation is orthonormal to LONG-double rounding (unit quaternion -> matrix in long double)"""
    LD = xprec.LD
    q = rng.normal(0, 1, 4).astype(LD)
    q /= np.sqrt((q * q).sum())
    w, x, y, z = q
    P = np.eye(4, dtype=LD)
    P[:3, :3] = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=LD)
    v = rng.normal(0, 1, 3)
    P[:3, 3] = (tnorm * v / np.linalg.norm(v)).astype(LD)
    return P


@pytest.mark.parametrize("plane,robust", FLAGS)
@pytest.mark.parametrize("tnorm,W", [(0.0, 0.0), (1.0, 0.0), (1e2, 0.0), (1e4, 0.0), (0.0, 1e2), (1e2, 1e4)])
def test_centred_moment_expansion_equals_the_direct_rows_in_long_double(plane, robust, tnorm, W):
    """The algebra of csrc/linearize.hip — moments of u' about the relative translation, H_ss = R6^T S R6, H_sd = -R6^T (S - X) L^T,
    H_dd = L (S - X - X^T + Y) L^T, g = [R6^T v ; -L v] — evaluated in long double against the direct long-double sums of the rows, on poses
    that are orthonormal to long-double rounding.  Nothing in the expansion cancels, so H without the robust weight agrees to long-double
    rounding whatever |t| and W: 2^-64 x 1024 (pairwise sums of 4000 terms and a dozen roundings per term, against pieces that may
    themselves cancel by a factor of ~sqrt(N)).  The residual is rounded once where p~ is formed, differently in the world frame and in the
    dst frame: g, the cost and the robust weights inherit that relative (|t| + W + 1) / |r| ~ extent / noise on top."""
    rng = np.random.default_rng(77)
    N = 4000
    LD = xprec.LD
    Pd = _ld_pose(rng, 0.7)
    Rel = _ld_pose(rng, tnorm)
    Ps = Pd @ Rel
    p = (rng.normal(0, lincases.SPREAD, (N, 3)) + W * np.array([0.6, 0.0, 0.8])).astype(LD)
    n = rng.normal(0, 1, (N, 3)); n /= np.linalg.norm(n, axis=1, keepdims=True)
    q = (p @ Rel[:3, :3].T + Rel[:3, 3]) + rng.normal(0, lincases.NOISE, (N, 3)).astype(LD)
    a = np.float32(lincases.NOISE)
    ref = xprec.edge_block(p, q, n, Ps, Pd, a, plane, robust)
    got = xprec.centred_blocks(p, q, n, Ps, Pd, a, plane, robust)
    ld_eps = LD(2.0) ** -64
    clean = 1024 * ld_eps
    resid = clean * (1 + 64 * (tnorm + W + 1) / lincases.NOISE)   # the once-rounded p~ against the residual it leaves, coherent over sqrt(N) = 64
    worst = {}
    for name, i, j in xprec.PIECES:
        A, B = got[0][3 * i:3 * i + 3, 3 * j:3 * j + 3], ref[0][3 * i:3 * i + 3, 3 * j:3 * j + 3]
        worst[name] = np.abs(A - B).max() / np.abs(B).max()
        assert worst[name] <= (resid if robust else clean), (name, float(worst[name]))
    for i in range(4):
        worst["g%d" % i] = np.abs(got[1][3 * i:3 * i + 3] - ref[1][3 * i:3 * i + 3]).max() / np.abs(ref[1][3 * i:3 * i + 3]).max()
        assert worst["g%d" % i] <= resid, (i, float(worst["g%d" % i]))
    assert abs(got[2] - ref[2]) <= resid * abs(ref[2])
    print("centred vs direct, long double (plane=%d robust=%d |t|=%g W=%g): H %.1e  g %.1e  cost %.1e" % (
        plane, robust, tnorm, W, max(float(v) for k, v in worst.items() if k[0] == "H"), max(float(v) for k, v in worst.items() if k[0] == "g"),
        float(abs(got[2] - ref[2]) / abs(ref[2]))))


def oracle_error_bound(kw, piece, plane, robust):
    """What rounding analysis allows the fp64 oracle on a sweep case (lincases.make_case keywords), relative to the piece's largest entry:
      * every piece: a serial sum of N terms with ~32 roundings each, (N + 32) eps of the sum of magnitudes — times sqrt(N) where the piece
        is a sum of both signs (the off-diagonal pieces, g);
      * whatever depends on the residual (g, the cost, and through the robust weight everything): the residual is a difference of
        world coordinates of size `extent`, each the end of ~13 roundings of that size (two rotated and translated points and their
        difference) with rotation entries that carry ~12 more from the quaternion round trip — 32 eps extent in all, largely common to
        all correspondences (the poses' rounding), so it adds up over N terms against a random sum of sqrt(N):
        32 sqrt(N) eps extent / min(noise, a);
      * the robust cost 2 a^2 (sqrt(1 + s / a^2) - 1) cancels for a >> |r|: 4 eps (1 + a^2 / noise^2)."""
    N = kw.get("N", lincases.N_BASE)
    unit = kw.get("unit", 1.0)
    rootn = np.sqrt(N)
    b = (N + 32) * EPS * (1.0 if (piece == "cost" or (piece[0] == "H" and piece[1] == piece[2])) else rootn)
    if piece[0] != "H" or robust:
        extent = (kw.get("tnorm", 0.0) + kw.get("W", 0.0) + 1.0) * unit
        af = kw.get("a_factor", 1.0) if robust else 1.0
        b += 32 * rootn * EPS * extent / (min(1.0, af) * lincases.NOISE * unit)
        if robust and piece == "cost":
            b += 4 * EPS * (1 + af * af)
    return b


@pytest.mark.parametrize("family", sorted(lincases.FAMILIES))
def test_oracle_error_on_the_sweep_cases_is_what_rounding_predicts(orc, family):
    """The bar of the GPU sweep is the oracle's own error, so a wrong oracle would make it vacuous: on every (base-size) case of the sweep the
    oracle's error against the extended reference stays under oracle_error_bound().  Observed: H 1e-14 (robust off), g from 1e-12 at the
    origin to 3e-7 at |t| = 1e4 / W = 1e4 (the c-form / world-frame residual)."""
    for fam, name, kw in lincases.all_cases():
        if fam != family:
            continue
        c = lincases.make_case(name, **kw)
        p, q, n = lincases.gathered(c)
        for plane, robust in FLAGS:
            ref = xprec.edge_block(p, q, n, c["poses"][1], c["poses"][0], c["a"], plane, robust)
            err = xprec.piece_errors(xprec.unpack(lincases.oracle_block(orc, c, plane, robust)), ref)
            line = []
            for piece, v in err.items():
                zero_ref = (piece == "cost" and ref[2] == 0) or (piece[0] == "g" and not np.any(ref[1][3 * int(piece[1]):3 * int(piece[1]) + 3]))
                if zero_ref:
                    continue   # an exactly-zero reference piece: the sweep demands an exact zero of the kernel, whatever the oracle gives
                bound = oracle_error_bound(kw, piece, plane, robust)
                line.append("%s %.0e" % (piece, v))
                assert v <= bound, (name, plane, robust, piece, v, bound)
            print("%-26s plane=%d robust=%d  oracle error: %s" % (name, plane, robust, " ".join(line)))


def test_normal_check_accepts_eigh_and_rejects_a_microradian():
    """tests/normcheck.py on the CPU: numpy's own normals of brute-force 10-NN sets pass; the same normals turned by 1e-6 rad — five digits
    beyond what the 1e-9 comparisons of the suite can see — fail."""
    import normcheck
    rng = np.random.default_rng(3)
    pts = rng.normal(0, 0.1, (400, 3)) * [1.0, 1.0, 0.2]
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    knn = np.argsort(d2, axis=1, kind="stable")[:, :10].astype(np.int32)
    nb = pts[knn]
    d = nb - nb.mean(axis=1, keepdims=True)
    lam, V = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    nrm = V[:, :, 0] * np.where(V[:, 2, 0] > 0, -1.0, 1.0)[:, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    normcheck.check(pts, knn, nrm, "numpy eigh")
    turned = nrm + 1e-6 * V[:, :, 1]
    turned /= np.linalg.norm(turned, axis=1, keepdims=True)
    turned *= np.where(turned[:, 2:3] > 0, -1.0, 1.0)
    with pytest.raises(AssertionError):
        normcheck.check(pts, knn, turned, "turned by 1e-6")
