"""CPU (-m "not gpu"): the plane-to-plane objective's reference (tests/gicpref.py) is checked against central differences with the weight
frozen, against the point-to-point rows at epsilon = 1, against the closed forms of the weight (agreeing normals; the kernel's Woodbury form;
a missing normal on either side), and the claim the objective is added for is tested: started off the truth on two independent samplings of
one curved surface, a registration over the plane-to-plane rows at epsilon = 1e-3 ends closer to the truth than one over the point-to-plane
rows, in rotation and in point displacement."""
import numpy as np
import pytest

import gicpref
import lincases
import matchref
import symcases
import symref
import xprec
from mvicp import synth
from mvicp import lib as mlib

LD = xprec.LD
U64 = LD(2.0) ** -64


def _exp6(d):
    """exp of [upsilon, omega] as a 4x4 (first order in upsilon is all the central difference needs)"""
    T = np.eye(4, dtype=LD)
    w = np.asarray(d[3:], dtype=np.float64)
    T[:3, :3] = synth.so3_exp(w).astype(LD)
    T[:3, 3] = np.asarray(d[:3], dtype=LD) + np.cross(w, np.asarray(d[:3], dtype=np.float64)).astype(LD) / 2
    return T


def _ld_pose(rng, tnorm):
    """a pose whose rotation is orthonormal to long-double rounding"""
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


def test_rows_agree_with_central_differences_with_the_weight_frozen():
    """W = G G^T is held at the evaluation poses; J (12 columns: ups_s, om_s, ups_d, om_d under T <- T exp(delta)) of the three rows G^T f
    against (G^T f(+h) - G^T f(-h)) / 2h in long double, h = 1e-6: the truncation error is h^2 x third derivatives ~ 1e-12 relative to rows of
    size 1, so 1e-10 leaves two digits.  Printed, not asserted: how far the gradient of s / 2 with W MOVING is from the frozen one, J^T W f —
    the term the Gauss-Newton form drops; it is of the order of |f|^2 / eps against |f|."""
    eps = 1e-3
    case = symcases.make_case("fd", seed=3, N=200, tnorm=1.0)
    p, q, nq, npn = symcases.gathered(case)
    Pd, Ps = case["poses"].astype(LD)
    f, J, W, _, _ = gicpref.rows(p, q, nq, npn, Ps, Pd, 1.0, eps, False)
    lam, V = np.linalg.eigh(np.transpose(W.astype(np.float64), (2, 0, 1)))
    G = np.transpose(V * np.sqrt(lam)[:, None, :], (1, 2, 0)).astype(LD)          # (3, 3, N): any fixed factor serves, both sides use the same
    Gt = lambda v: (G * v[:, None, :]).sum(axis=0)                                 # noqa: E731   G^T v per correspondence

    def half_s(Ps_, Pd_):
        f_, _, W_, _, _ = gicpref.rows(p, q, nq, npn, Ps_, Pd_, 1.0, eps, False)
        return ((W_ * f_[None, :, :]).sum(axis=1) * f_).sum(axis=0) / 2

    h = 1e-6
    worst = dropped = 0.0
    Wf = (W * f[None, :, :]).sum(axis=1)
    for k in range(12):
        d = np.zeros(6); d[k % 6] = h
        a, b = ((Ps @ _exp6(d), Pd), (Ps @ _exp6(-d), Pd)) if k < 6 else ((Ps, Pd @ _exp6(d)), (Ps, Pd @ _exp6(-d)))
        fd = (Gt(gicpref.residual(p, q, nq, npn, *a)) - Gt(gicpref.residual(p, q, nq, npn, *b))) / (2 * h)
        worst = max(worst, float(np.abs(fd - Gt(J[k])).max()))
        frozen = (J[k] * Wf).sum(axis=0)
        dropped = max(dropped, float(np.abs((half_s(*a) - half_s(*b)) / (2 * h) - frozen).max() / np.abs(frozen).max()))
    print("gicp rows against central differences, W frozen: %.1e;  the dropped dW term against the frozen gradient: %.1e" % (worst, dropped))
    assert worst <= 1e-10


@pytest.mark.parametrize("robust", [1, 0])
def test_epsilon_one_is_point_to_point(robust):
    """At epsilon = 1, S = 2 I and W = I exactly.  Against xprec.edge_block(plane = 0) on poses orthonormal to long-double rounding: the cost, the
    whole of g and every block of H that does not involve om_d are POINT's to long-double rounding.  The om_d blocks are NOT POINT's: f is the
    residual in the destination frame, f = R_d^T e, which turns with the destination, so its om_d rows are [p~]x = [q]x + [f]x where the
    world-frame residual e of POINT has R_d [q]x.  The extra term [f]x changes nothing in g (f x f = 0) and H by terms of first order in f; the
    contract's J_f (include/mvicp.h) is the one that reduces to PLANE as epsilon -> 0, where the normal turns with the destination too.  So for
    the om_d blocks the assertion is the exact relation: the block equals the sums of POINT's own rows with R_d [f]x added to their om_d
    columns.  The size of the difference from plain POINT is printed.
    Bound: both sides share e bit for bit; what differs is the order of the products, summed pairwise over N terms of either sign:
    64 x 2^-64 x log2(N) x sqrt(N)."""
    rng = np.random.default_rng(41)
    N = 4000
    Pd = _ld_pose(rng, 0.7)
    Rel = _ld_pose(rng, 1.0)
    Ps = Pd @ Rel
    p = rng.normal(0, lincases.SPREAD, (N, 3)).astype(LD)
    nq = rng.normal(0, 1, (N, 3)); npn = rng.normal(0, 1, (N, 3))
    q = (p @ Rel[:3, :3].T + Rel[:3, 3]) + rng.normal(0, lincases.NOISE, (N, 3)).astype(LD)
    a = np.float32(lincases.NOISE)
    got = gicpref.edge_block(p, q, nq, npn, Ps, Pd, a, 1.0, robust)
    ref = xprec.edge_block(p, q, None, Ps, Pd, a, 0, robust)
    # POINT's rows with the destination-frame term added
    r, J, corr, _ = xprec.rows(p, q, None, Ps, Pd, a, 0, robust)
    f = Pd[:3, :3].T @ r
    J = J.copy()
    for c in range(3):
        ec = np.zeros((3, N), dtype=LD); ec[c] = 1
        J[9 + c] += Pd[:3, :3] @ xprec._cross(f, ec)
    Jc = np.ascontiguousarray((J * corr).reshape(12, -1))
    Hx = np.array([[xprec._psum(Jc[i] * Jc[j]) for j in range(12)] for i in range(12)], dtype=LD)
    bound = 64 * U64 * np.log2(N) * np.sqrt(N)
    raw = 0.0
    for name, i, j in xprec.PIECES:
        A = got[0][3 * i:3 * i + 3, 3 * j:3 * j + 3]
        B = (Hx if j == 3 else ref[0])[3 * i:3 * i + 3, 3 * j:3 * j + 3]
        assert np.abs(A - B).max() <= bound * np.abs(B).max(), (name, float(np.abs(A - B).max() / np.abs(B).max()))
        if j == 3:
            P = ref[0][3 * i:3 * i + 3, 3 * j:3 * j + 3]
            raw = max(raw, float(np.abs(A - P).max() / np.abs(P).max()))
    for i in range(4):
        A, B = got[1][3 * i:3 * i + 3], ref[1][3 * i:3 * i + 3]
        assert np.abs(A - B).max() <= bound * np.abs(B).max(), ("g%d" % i, float(np.abs(A - B).max() / np.abs(B).max()))
    assert abs(got[2] - ref[2]) <= bound * abs(ref[2])
    print("epsilon = 1, robust=%d: cost, g and the blocks without om_d are POINT's; the om_d blocks differ from POINT's by %.1e (the [f]x term)" % (robust, raw))
    assert raw > 1e3 * float(bound)      # (the difference is the term above, not rounding)


@pytest.mark.parametrize("robust", [1, 0])
@pytest.mark.parametrize("eps", [1e-3, 1.0])
@pytest.mark.parametrize("tnorm,W", [(0.0, 0.0), (1.0, 0.0), (1e2, 0.0), (0.0, 1e2)])
def test_centred_moment_expansion_equals_the_direct_rows_in_long_double(robust, eps, tnorm, W):
    """The algebra of csrc/linearize_gicp.hip (gicpref.centred_blocks) against the direct rows, both in long double on poses orthonormal to
    long-double rounding.  Bounds, those of the same test of the symmetric objective (tests/test_sym_cpu.py) plus the weight's own: with
    clean = 1024 x 2^-64 and extent = |t| + W + 1, the residual is rounded once where p~ is formed, differently in the two forms, by
    2^-64 extent — against the om_d rows' [p~]x of size >= the spread in H without the robust weight, and against the residual itself,
    coherent over sqrt(N) = 64, in g, the cost and the robust weights — and the direct rows' inverse of S is good to 64 x 2^-64 / eps
    (test_weight_closed_forms)."""
    rng = np.random.default_rng(78)
    N = 4000
    Pd = _ld_pose(rng, 0.7)
    Rel = _ld_pose(rng, tnorm)
    Ps = Pd @ Rel
    p = (rng.normal(0, lincases.SPREAD, (N, 3)) + W * np.array([0.6, 0.0, 0.8])).astype(LD)
    nq = rng.normal(0, 1, (N, 3)); nq /= np.linalg.norm(nq, axis=1, keepdims=True)
    npn = rng.normal(0, 1, (N, 3)) * 2.0
    nq[:40] = 0.0; npn[20:60] = 0.0
    q = (p @ Rel[:3, :3].T + Rel[:3, 3]) + rng.normal(0, lincases.NOISE, (N, 3)).astype(LD)
    a = np.float32(lincases.NOISE)
    ref = gicpref.edge_block(p, q, nq, npn, Ps, Pd, a, eps, robust)
    got = gicpref.centred_blocks(p, q, nq, npn, Ps, Pd, a, eps, robust)
    clean = 1024 * U64
    winv = 64 * U64 / LD(eps)
    resid = clean * (1 + 64 * (tnorm + W + 1) / lincases.NOISE) + winv
    rows_bound = clean * (1 + (tnorm + W + 1) / lincases.SPREAD) + winv
    worst = {}
    for name, i, j in xprec.PIECES:
        A, B = got[0][3 * i:3 * i + 3, 3 * j:3 * j + 3], ref[0][3 * i:3 * i + 3, 3 * j:3 * j + 3]
        worst[name] = np.abs(A - B).max() / np.abs(B).max()
        assert worst[name] <= (resid if robust else rows_bound), (name, float(worst[name]))
    for i in range(4):
        worst["g%d" % i] = np.abs(got[1][3 * i:3 * i + 3] - ref[1][3 * i:3 * i + 3]).max() / np.abs(ref[1][3 * i:3 * i + 3]).max()
        assert worst["g%d" % i] <= resid, (i, float(worst["g%d" % i]))
    assert abs(got[2] - ref[2]) <= resid * abs(ref[2])
    print("gicp centred vs direct, long double (robust=%d eps=%g |t|=%g W=%g): H %.1e  g %.1e  cost %.1e" % (
        robust, eps, tnorm, W, max(float(v) for k, v in worst.items() if k[0] == "H"), max(float(v) for k, v in worst.items() if k[0] == "g"),
        float(abs(got[2] - ref[2]) / abs(ref[2]))))


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=0))


def test_weight_closed_forms():
    """In long double, at epsilon = 1e-3 and 1e-4.  (i) Agreeing unit normals: W = eps I + (1 - eps) n n^T.  (ii) Any two normals, of any length and
    sign: the form the kernel evaluates, W = eps I + kappa [(1 + eps)(a a^T + b b^T) + c d (a b^T + b a^T)] with a, b the normalised normals,
    d = a . b, c = 1 - eps, kappa = eps c / (4 eps + c^2 |a x b|^2); W is symmetric with eigenvalues in [eps, 1].  Bound: S is rounded to 2^-64
    of entries of size 2 and its smallest eigenvalue is 2 eps, so its inverse by cofactors is good to a few 2^-64 / eps: 64 x 2^-64 / eps."""
    rng = np.random.default_rng(5)
    N = 500
    for eps in (1e-3, 1e-4):
        bound = float(64 * U64 / LD(eps))
        n = rng.normal(0, 1, (3, N))
        nl = _unit(n.astype(LD))
        W = gicpref.weight(n.astype(LD), (-2.5 * n).astype(LD), eps)        # the same direction: another sign, another length
        want = LD(eps) * np.eye(3, dtype=LD)[:, :, None] + (1 - LD(eps)) * nl[:, None, :] * nl[None, :, :]
        err = float(np.abs(W - want).max())
        assert err <= bound, (eps, err)
        a, b = (rng.normal(0, 1, (3, N)) * 3.0).astype(LD), (rng.normal(0, 1, (3, N)) * 0.1).astype(LD)
        b[:, :50] = a[:, :50] * LD(-0.5) + (rng.normal(0, 1e-7, (3, 50))).astype(LD)   # nearly parallel pairs: Delta close to 4 eps
        W = gicpref.weight(a, b, eps)
        ah, bh = _unit(a), _unit(b)
        e, c = LD(eps), 1 - LD(eps)
        d = (ah * bh).sum(axis=0)
        z = xprec._cross(ah, bh)
        kappa = e * c / (4 * e + c * c * (z * z).sum(axis=0))
        outer = lambda x, y: x[:, None, :] * y[None, :, :]                  # noqa: E731
        want = e * np.eye(3, dtype=LD)[:, :, None] + kappa * ((1 + e) * (outer(ah, ah) + outer(bh, bh)) + c * d * (outer(ah, bh) + outer(bh, ah)))
        err2 = float(np.abs(W - want).max())
        assert err2 <= bound, (eps, err2)
        lam = np.linalg.eigvalsh(np.transpose(W.astype(np.float64), (2, 0, 1)))
        assert lam.min() >= eps * (1 - 1e-9) and lam.max() <= 1 + 1e-12 and np.array_equal(W, np.transpose(W, (1, 0, 2)))
        print("eps=%g: agreeing normals %.1e, Woodbury form %.1e (bound %.1e); eigenvalues in [%.6g, %.6g]" % (eps, err, err2, bound, lam.min(), lam.max()))


@pytest.mark.parametrize("robust", [1, 0])
def test_zero_normals_mean_the_identity_covariance_on_that_side(robust):
    """n_q = 0 on some rows, n_p = 0 on others, both on a few, a NaN normal on one: the block is finite and equals the sums over rows whose weight
    is written out for C = I on that side — W = eps I + eps (1 - eps) / (1 + eps) n n^T with the other side's unit normal, W = eps I with
    neither — to the bound of the test above."""
    eps = 1e-3
    case = symcases.make_case("zero normals", seed=12, N=600)
    p, q, nq, npn = symcases.gathered(case)
    nq, npn = nq.copy(), npn.copy()
    nq[0:200:3] = 0.0
    npn[1:200:3] = 0.0
    nq[300:310] = 0.0; npn[300:310] = 0.0
    nq[400, 1] = np.nan
    Pd, Ps = case["poses"]
    f, J, W, w, hr = gicpref.rows(p, q, nq, npn, Ps, Pd, case["a"], eps, robust)
    e = LD(eps)
    nu = _unit(np.where(np.any(npn != 0, axis=1), 1.0, np.nan)[None, :] * (xprec._ld(Pd)[:3, :3].T @ (xprec._ld(Ps)[:3, :3] @ xprec._ld(npn).T)))
    nql = _unit(xprec._ld(np.where(np.isfinite(nq).all(axis=1, keepdims=True) & np.any(nq != 0, axis=1, keepdims=True), nq, np.nan)).T)
    bound = float(64 * U64 / e)
    checked = 0
    for k in range(len(p)):
        has_q, has_p = bool(np.isfinite(nql[:, k]).all()), bool(np.isfinite(nu[:, k]).all())
        if has_q and has_p:
            continue
        want = e * np.eye(3, dtype=LD)
        for has, n in ((has_q, nql[:, k]), (has_p, nu[:, k])):
            if has:
                want = want + e * (1 - e) / (1 + e) * np.outer(n, n)
        assert np.abs(W[:, :, k] - want).max() <= bound, k
        checked += 1
    assert checked >= 140
    H, g, c = gicpref.edge_block(p, q, nq, npn, Ps, Pd, case["a"], eps, robust)
    assert np.isfinite(H.astype(np.float64)).all() and np.isfinite(g.astype(np.float64)).all() and np.isfinite(float(c))
    blk = gicpref.blocks_fp64(p, q, nq, npn, Ps, Pd, case["a"], eps, robust)
    assert np.isfinite(blk).all()
    err = gicpref.piece_errors(gicpref.unpack(blk), (H, g, c))
    print("zero normals, robust=%d: %d rows with a missing normal; fp64 yardstick's worst piece %.1e" % (robust, checked, max(err.values())))
    assert max(err.values()) <= 1e-9


def _plane_fp64(p, q, nq, Ps, Pd, a, robust):
    """the point-to-plane rows of xprec, summed to a 91-block in fp64"""
    H, g, c = xprec.edge_block(p, q, nq, Ps, Pd, a, 1, robust)
    return np.concatenate([H[np.triu_indices(12)].astype(np.float64), g.astype(np.float64), [float(c)]])


def host_registration(cl, objective, eps=1e-3, cutoff_spacings=3.0, rounds=25):
    """25 rounds of {brute-force NN with the cutoff rule; mvicp_lm_solve over a numpy evaluator} on the pair of matchref.e2e_clouds, dst fixed at
    the identity, src started 3 degrees and one spacing off the truth (tests/test_sym_cpu.py's loop).  objective: "plane", "symmetric", "gicp".
    -> final pose of src"""
    src, dst, sn, dn = cl["src"], cl["dst"], cl["src_nrm"], cl["dst_nrm"]
    P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
    for _ in range(rounds):
        first, second, a = symref.nn_cutoff(src, P[1], dst, P[0], cutoff_spacings * cl["spacing"])
        p, q, nq, npn = src[first], dst[second], dn[second], sn[first]

        def evaluate(poses):
            if objective == "gicp":
                return gicpref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], a, eps, True)[None, :]
            if objective == "symmetric":
                return symref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], a, True)[None, :]
            return _plane_fp64(p, q, nq, poses[1], poses[0], a, True)[None, :]

        P, _ = mlib.lm_solve_host(2, [1], [0], P, [1, 0], mlib.PARAM_SOPHUS_SE3, evaluate, 50)
    return P[1]


@pytest.mark.parametrize("partial", [False, True])
def test_gicp_registration_ends_closer_to_the_truth_than_point_to_plane(partial):
    """The two clouds are independent samplings of one curved surface with analytic normals.  Asserted: at epsilon = 1e-3 the plane-to-plane
    registration ends closer to the truth than the point-to-plane one, in rotation and in the largest displacement of a source point, on the
    full-overlap and on the partial-overlap pair.  A numpy prototype gave 0.0011 deg / 0.0033 spacings against 0.0315 / 0.0549 (full) and
    0.0048 / 0.0095 against 0.0814 / 0.109 (partial).  The symmetric objective's figures are printed alongside."""
    cl = matchref.e2e_clouds(partial)
    got = {}
    for objective in ("plane", "symmetric", "gicp"):
        got[objective] = symref.distance_to_truth(host_registration(cl, objective), cl["truth"], cl["src"], cl["spacing"])
    print("partial=%s  " % partial + "  |  ".join("%s ends %.4f deg, %.4f spacings" % (k, v[0], v[1]) for k, v in got.items())
          + "  (plane / gicp: %.1f, %.1f)" % (got["plane"][0] / got["gicp"][0], got["plane"][1] / got["gicp"][1]))
    assert got["gicp"][0] < got["plane"][0] and got["gicp"][1] < got["plane"][1], got


# ---------------------------------------------------------------- the predicate of P(n): 2^-1022 <= n . n < inf on the fp64 value
def test_a_subnormal_n_dot_n_is_a_missing_normal_and_why():
    """tests/gicpcases.py's subnormal band: rows scaled to lengths 2^-536 ... 2^-512, so n . n computed in fp64 is a subnormal number with 2 to 50 bits.
    (i) What the predicate `n . n > 0` gave there, with the kernel's operation order emulated in numpy fp64 (gicpcases.kernel_unit_fp64): a^ is
    off unit length by the relative rounding of n . n, up to 2^-2 — and W = eps I + kappa [...] is off by as much, against a bar that is 32 x an
    fp64 evaluation's 1e-13.  A reference that normalises in long double does not see it: that was a band the specification did not cover.
    (ii) The rule now: P(n) = 0 unless 2^-1022 <= n . n < inf as computed in fp64 (include/mvicp.h).  gicpref takes the predicate on the fp64
    value whatever type it computes in, so these rows, rows whose n . n overflows fp64 (1e200: finite in long double) or underflows to 0
    (1e-200: positive in long double), and NaN / Inf rows give exactly the sums of the same case with those normals set to 0."""
    import gicpcases
    eps = 1e-3
    case = symcases.make_case("subnormal", seed=1600, N=2001, M=3000, chunk=512)
    unit_nor = case["nor"].copy()
    rows = gicpcases.subnormal(case)
    scaled = case["nor"][rows[0]]
    with np.errstate(under="ignore"):
        nn = (scaled * scaled).sum(axis=1)
    assert np.all(nn > 0) and np.all(nn < gicpref.TINY)
    u = gicpcases.kernel_unit_fp64(scaled)
    off = np.abs((u * u).sum(axis=1) - 1)
    away = np.abs(u - unit_nor[rows[0]]).max(axis=1)          # (the rows were unit vectors before the scaling)
    print("subnormal n . n, predicate `> 0`: |a^|^2 - 1 up to %.1e (over 1e-6 on %d of %d rows); a^ away from n / |n| by up to %.1e" % (
        off.max(), int((off > 1e-6).sum()), len(off), away.max()))
    assert off.max() > 1e-2 and (off > 1e-6).sum() > 50           # the hole: far beyond any bar
    assert not gicpref.has_normal(scaled.T).any() and gicpref.has_normal(unit_nor.T).all()
    for edit in (None, gicpcases.nonfinite):
        c = case if edit is None else symcases.make_case("nonfinite", seed=1700, N=2001, M=3000, chunk=512)
        r = rows if edit is None else edit(c)
        z = gicpcases.zeroed(c, r)
        Pd, Ps = c["poses"]
        for robust in (1, 0):
            got, want = gicpref.edge_block(*symcases.gathered(c), Ps, Pd, c["a"], eps, robust), gicpref.edge_block(*symcases.gathered(z), Ps, Pd, c["a"], eps, robust)
            assert np.array_equal(gicpref.pack(*got), gicpref.pack(*want)) and np.all(np.isfinite(gicpref.pack(*got).astype(np.float64)))
            assert np.array_equal(gicpref.blocks_fp64(*symcases.gathered(c), Ps, Pd, c["a"], eps, robust), gicpref.blocks_fp64(*symcases.gathered(z), Ps, Pd, c["a"], eps, robust))
            got_c = gicpref.centred_blocks(*symcases.gathered(c), Ps, Pd, c["a"], eps, robust)
            assert np.array_equal(gicpref.pack(*got_c), gicpref.pack(*gicpref.centred_blocks(*symcases.gathered(z), Ps, Pd, c["a"], eps, robust)))


# ---------------------------------------------------------------- plane-to-plane solves that reject steps (tests/gicpreject.py)
@pytest.fixture(scope="module")
def gicprej_world(orc):
    import lmreject
    pb, corr, w = lmreject.lists_at_init(orc)
    return pb, corr, w


def _gicprej_cases():
    import gicpreject
    return [pytest.param(c, id=gicpreject.case_id(c)) for c in gicpreject.CASES]


@pytest.mark.parametrize("case", _gicprej_cases())
def test_gicp_reference_solves_reject_as_recorded(gicprej_world, case, monkeypatch, capfd):
    """The reference of tests/test_gpu_gicp_rejected.py — the host solve over gicpref.blocks_fp64 at epsilon = 1e-3 — from the starts of
    tests/gicpreject.py: its iterations and successful steps are the recorded ones, it stops on the function tolerance (the one AT_LIMIT case:
    at the iteration limit), a must-reject case rejects at least two steps, and no accept / reject decision of any case is closer than 1e-6
    to min_relative_decrease (the recorded margins hold): device blocks that agree with the fp64 rows to 1e-11 cannot flip a decision, so the
    GPU test may assert equal COUNTS."""
    import gicpreject
    pb, corr, w = gicprej_world
    P0, P, sm, rd = gicpreject.traced_reference_solve(pb, corr, w, case, 50, monkeypatch, capfd)
    margin = float(np.abs(rd - gicpreject.MIN_RELATIVE_DECREASE).min())
    rejected = int((rd <= gicpreject.MIN_RELATIVE_DECREASE).sum())
    print(gicpreject.case_id(case), sm["iterations"], "/", sm["successful_steps"], "termination", sm["termination"], "| rejected", rejected,
          "| min |relative_decrease - 1e-3| = %.3e" % margin)
    assert (sm["iterations"], sm["successful_steps"]) == gicpreject.MEASURED[case], sm
    assert sm["termination"] == (0 if case in gicpreject.AT_LIMIT else 3), sm
    assert rejected == sm["iterations"] - sm["successful_steps"] - (0 if case in gicpreject.AT_LIMIT else 1)
    if case in gicpreject.REJECTING:
        assert rejected >= 2, (sm, rd)
    else:
        assert rejected == 0, (sm, rd)
    assert margin > 1e-6 and margin >= gicpreject.MEASURED_MARGIN[case], (margin, rd)
    assert not np.array_equal(P, P0)


def test_gicp_rejecting_cases_cover_both_losses_and_both_rotation_parameterizations():
    import gicpreject
    R = gicpreject.REJECTING
    assert len(R) >= 4 and {c[1] for c in R} == {0, 1} and {mlib.PARAM_EIGEN_QUATERNION, mlib.PARAM_ANGLE_AXIS} <= {c[2] for c in R}, R


@pytest.mark.parametrize("case", _gicprej_cases())
def test_gicp_reference_solves_stop_at_the_iteration_limit(gicprej_world, case):
    import gicpreject
    pb, corr, w = gicprej_world
    _, _, sm = gicpreject.reference_solve(pb, corr, w, case, 3)
    assert sm["termination"] == 0 and sm["iterations"] == 3 and sm["evaluations"] == 4, sm
