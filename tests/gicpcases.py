"""Normal families for the plane-to-plane sweep (tests/test_gpu_gicp_accuracy.py, tests/test_gicp_cpu.py): edits of a symcases.make_case dict that
give the kernel the normals it exists for and the ones its contract names.  Test infrastructure only; numpy only.

symcases draws n_q and n_p as independent random unit vectors, so d = a^ . b^ is spread over [-1, 1].  Here:

  parallel   n_p = A^T R(theta) n_q on every pair of the case's list: A = R_d^T R_s from the case's poses in fp64, R(theta) a tilt by theta about
             a random axis perpendicular to n_q.  theta -> 0 and theta -> pi are the registration regime: Delta -> 4 eps, kappa at its largest.
  sign       a random half of the destination normals negated, and independently a random half of the source normals.
  length     every normal of both sides times 2^k, k uniform over the integers of [-500, 500] (n . n stays a normal fp64 number).
  subnormal  rows (about 300 of each side, a few pairs on both) times m 2^k, m uniform in [1, 2), k in [-536, -513]: n . n, as computed in fp64,
             lies in (0, 2^-1024), below the contract's predicate (include/mvicp.h: n . n >= 2^-1022), so the normal counts as missing.  (m: a unit
             vector times 2^k alone has n . n = 4^k to within rounding, which a subnormal sum often hits exactly.)
  nonfinite  rows with one NaN component, one +-Inf component, components of +-1e200 (n . n overflows) and of +-1e-200 (n . n underflows to 0).

Every edit works in place on case["nor"] (destination, frame 0) and case["snor"] (source, frame 1) and leaves the rest of the case alone."""
import numpy as np

THETAS = (0.0, 1e-8, 1e-4, 1e-2, np.pi - 1e-4, np.pi)
PARALLEL_EPSILONS = (1e-6, 1e-4, 1e-3, 1.0)
N_BAD = 300      # rows per side of the subnormal and nonfinite families
N_BOTH = 8       # pairs of the list that get a bad normal on both sides


def theta_name(theta):
    return "pi" + ("-%g" % (np.pi - theta) if theta < np.pi else "") if theta > 3 else "%g" % theta


def parallel(case, theta, seed=0):
    """n_p of every listed pair = A^T (cos(theta) n_q + sin(theta) m), m a random unit vector perpendicular to n_q"""
    rng = np.random.default_rng(31000 + seed)
    f, s = case["first"], case["second"]
    nq = case["nor"][s]
    m = np.cross(nq, rng.normal(0, 1, nq.shape))
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    tilted = np.cos(theta) * nq + np.sin(theta) * m
    Pd, Ps = case["poses"]
    A = Pd[:3, :3].T @ Ps[:3, :3]
    case["snor"][f] = tilted @ A          # rows: (A^T v)^T = v^T A
    return case


def sign(case, seed=0):
    rng = np.random.default_rng(32000 + seed)
    for key in ("nor", "snor"):
        flip = rng.random(len(case[key])) < 0.5
        assert 0 < flip.sum() < len(flip)
        case[key][flip] = -case[key][flip]
    return case


def length(case, seed=0):
    rng = np.random.default_rng(33000 + seed)
    for key in ("nor", "snor"):
        case[key] *= np.ldexp(1.0, rng.integers(-500, 501, len(case[key])))[:, None]
    return case


def bad_rows(case, seed=0):
    """-> (rows of case["nor"], rows of case["snor"]) for the subnormal / nonfinite families: N_BAD listed rows of each side (fewer on a short list),
    N_BOTH of them the two sides of the same pairs"""
    rng = np.random.default_rng(34000 + seed)
    f, s = case["first"], case["second"]
    n = len(f)
    k = min(N_BAD, n // 3)
    pick = rng.permutation(n)
    both, only_q, only_p = pick[:N_BOTH], pick[N_BOTH:k], pick[k:2 * k - N_BOTH]
    return np.concatenate([s[both], s[only_q]]), np.concatenate([f[both], f[only_p]])


def subnormal(case, seed=0):
    """-> the rows it scaled, as bad_rows gives them"""
    rng = np.random.default_rng(35000 + seed)
    rq, rp = bad_rows(case, seed)
    for key, rows in (("nor", rq), ("snor", rp)):
        case[key][rows] *= np.ldexp(rng.uniform(1.0, 2.0, len(rows)), rng.integers(-536, -512, len(rows)))[:, None]
    return rq, rp


def nonfinite(case, seed=0):
    """-> the rows it spoiled.  Four kinds in turn: a NaN component, a +-Inf component, +-1e200 in every component, +-1e-200 in every component."""
    rng = np.random.default_rng(36000 + seed)
    rq, rp = bad_rows(case, seed)
    for key, rows in (("nor", rq), ("snor", rp)):
        for i, r in enumerate(rows):
            kind, comp = i % 4, int(rng.integers(0, 3))
            sgn = np.where(rng.random(3) < 0.5, -1.0, 1.0)
            if kind == 0:
                case[key][r, comp] = np.nan
            elif kind == 1:
                case[key][r, comp] = sgn[0] * np.inf
            elif kind == 2:
                case[key][r] = sgn * 1e200
            else:
                case[key][r] = sgn * 1e-200
    return rq, rp


def zeroed(case, rows):
    """a copy of the case with the rows of bad_rows set to exactly 0"""
    out = dict(case, nor=case["nor"].copy(), snor=case["snor"].copy())
    out["nor"][rows[0]] = 0.0
    out["snor"][rows[1]] = 0.0
    return out


def kernel_unit_fp64(n):
    """csrc/linearize_gicp.hip's a^ with the predicate `alpha > 0 && alpha < inf` it had before the 2^-1022 rule, in numpy fp64 (plain products and sums
    for the kernel's fma chain: in the subnormal band the difference is one unit of 2^-1074, the size of the effect itself).  (N, 3) -> (N, 3)"""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        nn = n[:, 2] * n[:, 2] + (n[:, 1] * n[:, 1] + n[:, 0] * n[:, 0])
        ok = (nn > 0) & (nn < np.inf)
        r = 1.0 / np.sqrt(np.where(ok, nn, 1.0))
        return np.where(ok[:, None], n * r[:, None], 0.0)
