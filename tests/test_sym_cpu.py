"""CPU (-m "not gpu"): the symmetric objective's reference (tests/symref.py) is checked against central differences, the kernel's moment
formulation is proved equal to the direct world-frame rows in long double, the fp64 yardstick's own error is printed per family, and the
claim the objective is built for is tested: started off the truth on two independent samplings of one curved surface, a registration
over the symmetric rows ends closer to the truth than one over the point-to-plane rows, in rotation and in point displacement."""
import numpy as np
import pytest

import lincases
import matchref
import symcases
import symref
import xprec
from mvicp import synth
from mvicp import lib as mlib

LD = xprec.LD


def _exp6(d):
    """exp of [upsilon, omega] as a 4x4 (first order in upsilon is all the central difference needs: V(omega) upsilon ~ upsilon + O(|d|^2))"""
    T = np.eye(4, dtype=LD)
    w = np.asarray(d[3:], dtype=np.float64)
    T[:3, :3] = synth.so3_exp(w).astype(LD)
    T[:3, 3] = np.asarray(d[:3], dtype=LD) + np.cross(w, np.asarray(d[:3], dtype=np.float64)).astype(LD) / 2
    return T


def test_rows_agree_with_central_differences_of_the_residual():
    """J (12 columns: ups_s, om_s, ups_d, om_d under T <- T exp(delta)) against (r(+h) - r(-h)) / 2h in long double, h = 1e-6: the truncation
    error is h^2 x third derivatives ~ 1e-12 relative to rows of size 1, so 1e-10 leaves two digits.  Observed: 1.9e-13."""
    case = symcases.make_case("fd", seed=3, N=200, tnorm=1.0)
    p, q, nq, npn = symcases.gathered(case)
    Pd, Ps = case["poses"].astype(LD)
    _, J, _, _ = symref.rows(p, q, nq, npn, Ps, Pd, 1.0, False)
    h = 1e-6
    worst = 0.0
    for k in range(12):
        d = np.zeros(6); d[k % 6] = h
        if k < 6:
            rp = symref.residual(p, q, nq, npn, Ps @ _exp6(d), Pd); rm = symref.residual(p, q, nq, npn, Ps @ _exp6(-d), Pd)
        else:
            rp = symref.residual(p, q, nq, npn, Ps, Pd @ _exp6(d)); rm = symref.residual(p, q, nq, npn, Ps, Pd @ _exp6(-d))
        worst = max(worst, float(np.abs((rp - rm) / (2 * h) - J[k]).max()))
    print("symmetric rows against central differences: %.1e" % worst)
    assert worst <= 1e-10


def _ld_pose(rng, tnorm):
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


@pytest.mark.parametrize("robust", [1, 0])
@pytest.mark.parametrize("tnorm,W", [(0.0, 0.0), (1.0, 0.0), (1e2, 0.0), (1e4, 0.0), (0.0, 1e2), (1e2, 1e4)])
def test_centred_moment_expansion_equals_the_direct_rows_in_long_double(robust, tnorm, W):
    """The algebra of csrc/linearize_sym.hip against the direct world-frame rows, both in long double on poses orthonormal to long-double
    rounding — the bounds of the same test of the other two families (tests/test_xprec.py), with one difference: the symmetric ROWS contain
    the residual vector (the term (n_p x R_s^T e) / 2), which is rounded once where p~ is formed, differently in the world frame and in the
    dst frame, by 2^-64 (|t| + W + 1) against angular rows of size >= the cloud's spread.  So H without the robust weight agrees to
    1024 x 2^-64 x (1 + (|t| + W + 1) / spread); g, the cost and the robust weights carry that rounding against the residual itself,
    (|t| + W + 1) / noise, coherent over sqrt(N) = 64."""
    rng = np.random.default_rng(78)
    N = 4000
    Pd = _ld_pose(rng, 0.7)
    Rel = _ld_pose(rng, tnorm)
    Ps = Pd @ Rel
    p = (rng.normal(0, lincases.SPREAD, (N, 3)) + W * np.array([0.6, 0.0, 0.8])).astype(LD)
    nq = rng.normal(0, 1, (N, 3)); nq /= np.linalg.norm(nq, axis=1, keepdims=True)
    npn = rng.normal(0, 1, (N, 3)); npn /= np.linalg.norm(npn, axis=1, keepdims=True)
    q = (p @ Rel[:3, :3].T + Rel[:3, 3]) + rng.normal(0, lincases.NOISE, (N, 3)).astype(LD)
    a = np.float32(lincases.NOISE)
    ref = symref.edge_block(p, q, nq, npn, Ps, Pd, a, robust)
    got = symref.centred_blocks(p, q, nq, npn, Ps, Pd, a, robust)
    clean = 1024 * LD(2.0) ** -64
    resid = clean * (1 + 64 * (tnorm + W + 1) / lincases.NOISE)
    rows_bound = clean * (1 + (tnorm + W + 1) / lincases.SPREAD)
    worst = {}
    for name, i, j in xprec.PIECES:
        A, B = got[0][3 * i:3 * i + 3, 3 * j:3 * j + 3], ref[0][3 * i:3 * i + 3, 3 * j:3 * j + 3]
        worst[name] = np.abs(A - B).max() / np.abs(B).max()
        assert worst[name] <= (resid if robust else rows_bound), (name, float(worst[name]))
    for i in range(4):
        worst["g%d" % i] = np.abs(got[1][3 * i:3 * i + 3] - ref[1][3 * i:3 * i + 3]).max() / np.abs(ref[1][3 * i:3 * i + 3]).max()
        assert worst["g%d" % i] <= resid, (i, float(worst["g%d" % i]))
    assert abs(got[2] - ref[2]) <= resid * abs(ref[2])
    print("symmetric centred vs direct, long double (robust=%d |t|=%g W=%g): H %.1e  g %.1e  cost %.1e" % (
        robust, tnorm, W, max(float(v) for k, v in worst.items() if k[0] == "H"), max(float(v) for k, v in worst.items() if k[0] == "g"),
        float(abs(got[2] - ref[2]) / abs(ref[2]))))


def _ld_orthonormal(P):
    """the fp64 pose with its rotation made orthonormal to long-double rounding (three Newton-Schulz steps from a defect of a few 2^-52)"""
    P = np.asarray(P).astype(LD)
    R = P[:3, :3]
    for _ in range(3):
        R = R @ (3 * np.eye(3, dtype=LD) - R.T @ R) / 2
    P[:3, :3] = R
    return P


_CPU_FAMILIES = dict(symcases.FAMILIES, count=symcases.COUNTS, subset=symcases.SUBSETS)


@pytest.mark.parametrize("family", sorted(_CPU_FAMILIES))
def test_centred_equals_direct_on_every_family_and_the_fp64_yardstick_is_printed(family):
    """On every case of the GPU sweep (tests/symcases.py: the six conditioning families, the counts, the strict subsets) the moment formulation
    equals the direct world-frame rows to long-double rounding, EVERY piece (10 of H, 4 of g, the cost), robust on and off.  The two forms agree
    only as far as R_d^T is R_d^-1, so the case's fp64 poses are first made orthonormal to long-double rounding (the translations and all other
    inputs stay the fp64 values).  Bounds, those of the test above with this case's own figures: with clean = 1024 x 2^-64 and extent =
    |t| + W + 1, H without the robust weight to clean (1 + extent / spread) — the rows contain the once-rounded residual vector — and g, the cost
    and every robust piece to clean (1 + sqrt(N) extent / (min(1, a / noise) noise)): the rounding of p~ against the residual it leaves, coherent
    over the N correspondences, and against the scale a where a is the smaller (the robust weight is a function of r / a).  A piece whose reference
    is exactly zero (the zero family's g and cost) must be exactly zero.  The fp64 yardstick's error on the case as the GPU sees it is printed."""
    clean = 1024 * LD(2.0) ** -64
    for kw in _CPU_FAMILIES[family]:
        name = symcases.case_name(family, kw)
        case = symcases.make_case(name, seed=300, **{k: v for k, v in kw.items() if k != "chunk"})
        p, q, nq, npn = symcases.gathered(case)
        Pd, Ps = case["poses"]
        Pdl, Psl = _ld_orthonormal(Pd), _ld_orthonormal(Ps)
        extent = kw.get("tnorm", 0.0) + kw.get("W", 0.0) + 1.0
        rows_bound = clean * (1 + extent / lincases.SPREAD)
        for robust in (1, 0):
            af = min(1.0, kw.get("a_factor", 1.0)) if robust else 1.0
            resid = clean * (1 + np.sqrt(len(p)) * extent / (af * lincases.NOISE))
            ref = symref.edge_block(p, q, nq, npn, Psl, Pdl, case["a"], robust)
            got = symref.centred_blocks(p, q, nq, npn, Psl, Pdl, case["a"], robust)
            pieces = [(nm, got[0][3 * i:3 * i + 3, 3 * j:3 * j + 3], ref[0][3 * i:3 * i + 3, 3 * j:3 * j + 3], resid if robust else rows_bound) for nm, i, j in xprec.PIECES]
            pieces += [("g%d" % i, got[1][3 * i:3 * i + 3], ref[1][3 * i:3 * i + 3], resid) for i in range(4)]
            pieces.append(("cost", np.atleast_1d(got[2]), np.atleast_1d(ref[2]), resid))
            worst = {"H": 0.0, "g": 0.0, "c": 0.0}
            for nm, A, B, bound in pieces:
                den = np.abs(B).max()
                if den == 0:
                    assert not np.any(A), (name, robust, nm)
                    continue
                rel = float(np.abs(A - B).max() / den)
                worst[nm[0]] = max(worst[nm[0]], rel)
                assert rel <= bound, (name, robust, nm, rel, float(bound))
            if family == "zero":
                assert not np.any(ref[1]) and ref[2] == 0
            err = symref.piece_errors(symref.unpack(symref.blocks_fp64(p, q, nq, npn, Ps, Pd, case["a"], robust)), symref.edge_block(p, q, nq, npn, Ps, Pd, case["a"], robust))
            print("%-32s robust=%d  centred vs direct (long double): H %.1e g %.1e cost %.1e | fp64 yardstick: H %.1e  g %.1e  cost %.1e" % (
                name, robust, worst["H"], worst["g"], worst["c"],
                max(v for k, v in err.items() if k[0] == "H"), max(v for k, v in err.items() if k[0] == "g"), err["cost"]))


def _plane_fp64(p, q, nq, Ps, Pd, a, robust):
    """the point-to-plane rows of xprec, summed to a 91-block in fp64"""
    H, g, c = xprec.edge_block(p, q, nq, Ps, Pd, a, 1, robust)
    out = np.zeros(91)
    out[:78] = H[np.triu_indices(12)].astype(np.float64); out[78:90] = g.astype(np.float64); out[90] = float(c)
    return out


def host_registration(cl, symmetric, cutoff_spacings=3.0, rounds=25):
    """25 rounds of {brute-force NN with the cutoff rule; mvicp_lm_solve over a numpy evaluator} on the pair of matchref.e2e_clouds,
    dst fixed at the identity, src started 3 degrees and one spacing off the truth.  -> final pose of src"""
    src, dst, sn, dn = cl["src"], cl["dst"], cl["src_nrm"], cl["dst_nrm"]
    P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
    for _ in range(rounds):
        first, second, a = symref.nn_cutoff(src, P[1], dst, P[0], cutoff_spacings * cl["spacing"])
        p, q, nq, npn = src[first], dst[second], dn[second], sn[first]

        def evaluate(poses):
            if symmetric:
                return symref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], a, True)[None, :]
            return _plane_fp64(p, q, nq, poses[1], poses[0], a, True)[None, :]

        P, _ = mlib.lm_solve_host(2, [1], [0], P, [1, 0], mlib.PARAM_SOPHUS_SE3, evaluate, 50)
    return P[1]


@pytest.mark.parametrize("partial", [False, True])
def test_symmetric_registration_ends_closer_to_the_truth_than_point_to_plane(partial):
    """The behaviour the objective exists for.  The two clouds are independent samplings of one curved surface with analytic normals, so the
    point-to-plane residual does not vanish at the true pose; the symmetric one does to second order.  Asserted: the ordering, in rotation and
    in the largest displacement of a source point.  A numpy prototype gave 0.029-0.032 deg / 0.050-0.056 spacings (plane) against
    0.0045-0.0047 deg / 0.006 spacings (symmetric) on the full-overlap pair, 0.083 / 0.112 against 0.0042 / 0.008 on the partial one."""
    cl = matchref.e2e_clouds(partial)
    got = {}
    for symmetric in (False, True):
        P = host_registration(cl, symmetric)
        got[symmetric] = symref.distance_to_truth(P, cl["truth"], cl["src"], cl["spacing"])
    print("partial=%s  point-to-plane ends %.4f deg, %.4f spacings  |  symmetric ends %.4f deg, %.4f spacings  (ratios %.1f, %.1f)" % (
        partial, got[False][0], got[False][1], got[True][0], got[True][1], got[False][0] / got[True][0], got[False][1] / got[True][1]))
    assert got[True][0] < got[False][0] and got[True][1] < got[False][1], got


def _ld_inverse(M):
    """3x3 inverse by cofactors in long double (numpy's linalg has no long double)"""
    M = np.asarray(M, dtype=LD)
    C = np.array([[M[(i + 1) % 3, (j + 1) % 3] * M[(i + 2) % 3, (j + 2) % 3] - M[(i + 1) % 3, (j + 2) % 3] * M[(i + 2) % 3, (j + 1) % 3] for j in range(3)] for i in range(3)], dtype=LD)
    return C.T / (M[0] * C[0]).sum()


@pytest.mark.parametrize("robust", [1, 0])
def test_the_transpose_substitution_reduces_to_the_centred_blocks_for_a_rotation(robust):
    """tests/test_gpu_sym_accuracy.py holds the kernel at a destination that is no rotation to symref.centred_blocks, because that function writes
    R_d^T where the library (for a rotation) forms the true inverse.  Here: (i) `inv` really is the matrix in the place of R_d^-1 — handing in
    R_d^T gives the default's values bit for bit, handing in another matrix does not; (ii) for a rotation orthonormal to long-double rounding
    the true inverse and the transpose give the same blocks to the bound of the tests above, so for rotations the substituted reference is the
    one every other test uses; (iii) the fp64 variant (the GPU test's yardstick) is the same formulation: it agrees with the long-double one
    to fp64 rounding, printed, and within the N x 2^-52 x extent / noise that a coherent rounding of the residual can cost."""
    case = symcases.make_case("substitution", seed=77, N=513)
    p, q, nq, npn = symcases.gathered(case)
    Pd, Ps = _ld_orthonormal(case["poses"][0]), _ld_orthonormal(case["poses"][1])
    base = symref.centred_blocks(p, q, nq, npn, Ps, Pd, case["a"], robust)
    same = symref.centred_blocks(p, q, nq, npn, Ps, Pd, case["a"], robust, inv=Pd[:3, :3].T)
    assert all(np.array_equal(np.atleast_1d(a), np.atleast_1d(b)) for a, b in zip(base, same))
    other = symref.centred_blocks(p, q, nq, npn, Ps, Pd, case["a"], robust, inv=3 * Pd[:3, :3].T)
    assert not np.array_equal(other[0], base[0])
    true_inv = symref.centred_blocks(p, q, nq, npn, Ps, Pd, case["a"], robust, inv=_ld_inverse(Pd[:3, :3]))
    bound = 1024 * LD(2.0) ** -64 * (1 + np.sqrt(len(p)) * 2.0 / lincases.NOISE)     # (clean x coherent rounding of p~ against the residual, as above: extent = |t| + 1 <= 2)
    worst = 0.0
    for a, b in zip(true_inv, base):
        a, b = np.atleast_1d(a), np.atleast_1d(b)
        worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    print("true inverse against transpose, long double, robust=%d: %.1e (bound %.1e)" % (robust, worst, float(bound)))
    assert worst <= bound
    err = symref.piece_errors(symref.centred_blocks(p, q, nq, npn, Ps.astype(np.float64), Pd.astype(np.float64), case["a"], robust, ftype=np.float64),
                              symref.centred_blocks(p, q, nq, npn, Ps.astype(np.float64), Pd.astype(np.float64), case["a"], robust))
    print("fp64 variant against long double, robust=%d: worst piece %.1e" % (robust, max(err.values())))
    assert max(err.values()) <= len(p) * 2.0 ** -52 * 2.0 / lincases.NOISE
    # and for a destination that is no rotation the fp64 variant still is the long-double one to fp64 rounding (nothing cancels there)
    Pn = case["poses"][0].copy(); Pn[:3, :3] = 3.0 * Pn[:3, :3]
    err = symref.piece_errors(symref.centred_blocks(p, q, nq, npn, case["poses"][1], Pn, case["a"], robust, ftype=np.float64),
                              symref.centred_blocks(p, q, nq, npn, case["poses"][1], Pn, case["a"], robust))
    print("fp64 variant against long double at 3 R, robust=%d: worst piece %.1e" % (robust, max(err.values())))
    assert max(err.values()) <= len(p) * 2.0 ** -52


# ---------------------------------------------------------------- symmetric solves that reject steps (tests/symreject.py)
@pytest.fixture(scope="module")
def symrej_world(orc):
    import lmreject
    pb, corr, w = lmreject.lists_at_init(orc)
    return pb, corr, w


def _symrej_cases():
    import symreject
    return [pytest.param(c, id=symreject.case_id(c)) for c in symreject.CASES]


@pytest.mark.parametrize("case", _symrej_cases())
def test_symmetric_reference_solves_reject_as_recorded(symrej_world, case, monkeypatch, capfd):
    """The reference of tests/test_gpu_sym_rejected.py — the host solve over symref.blocks_fp64 — from the starts of tests/symreject.py: its
    iterations and successful steps are the recorded ones, it stops on the function tolerance, a must-reject case rejects at least two steps,
    and no accept / reject decision of any case is closer than 1e-6 to min_relative_decrease (the recorded margins hold): device blocks that
    agree with the fp64 rows to 1e-11 cannot flip a decision, so the GPU test may assert equal COUNTS."""
    import symreject
    pb, corr, w = symrej_world
    P0, P, sm, rd = symreject.traced_reference_solve(pb, corr, w, case, 50, monkeypatch, capfd)
    margin = float(np.abs(rd - symreject.MIN_RELATIVE_DECREASE).min())
    rejected = int((rd <= symreject.MIN_RELATIVE_DECREASE).sum())
    print(symreject.case_id(case), sm["iterations"], "/", sm["successful_steps"], "termination", sm["termination"], "| rejected", rejected,
          "| min |relative_decrease - 1e-3| = %.3e" % margin)
    assert (sm["iterations"], sm["successful_steps"]) == symreject.MEASURED[case] and sm["termination"] == 3, sm
    assert rejected == sm["iterations"] - sm["successful_steps"] - 1
    if case in symreject.REJECTING:
        assert rejected >= 2, (sm, rd)
    else:
        assert rejected == 0, (sm, rd)
    assert margin > 1e-6 and margin >= symreject.MEASURED_MARGIN[case], (margin, rd)
    assert not np.array_equal(P, P0)


@pytest.mark.parametrize("case", _symrej_cases())
def test_symmetric_reference_solves_stop_at_the_iteration_limit(symrej_world, case):
    import symreject
    pb, corr, w = symrej_world
    _, _, sm = symreject.reference_solve(pb, corr, w, case, 3)
    assert sm["termination"] == 0 and sm["iterations"] == 3 and sm["evaluations"] == 4, sm
