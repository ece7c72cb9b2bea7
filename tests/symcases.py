"""lincases.make_case for the symmetric objective (tests/test_sym_cpu.py, tests/test_gpu_sym_accuracy.py): the same two-frame, one-edge
problems plus what the symmetric kernel reads and lincases does not vary.  Test infrastructure only.

  * source normals of their own ("snor", per source point): random unit vectors, drawn from a stream of their own so that the lincases
    part of a case is what lincases makes for the same keywords; in the zero family three-bit components like the dst normals, so that
    the rotated source normal, the mean normal and every product with it stay exact;
  * a cloud size M > N: lincases makes `first` a strict subset only below 64 points, so for N >= 64 the source normal would never be
    gathered through a `first` that is not the identity.  With M, the clouds have M points and the list is a sorted random N-subset."""
import numpy as np

import lincases


def make_case(name, seed=1, N=lincases.N_BASE, M=None, **kw):
    """-> lincases.make_case's dict (clouds of max(N, 64) points, or of M > N points with an N-subset as the list) + "snor" """
    if M is None:
        case = lincases.make_case(name, seed=seed, N=N, **kw)
    else:
        assert M > N
        case = lincases.make_case(name, seed=seed, N=M, **kw)     # first = arange(M), second = the permutation dst is stored in
        perm = case["second"]
        rng = np.random.default_rng(seed + 5000)
        first = np.sort(rng.choice(M, N, replace=False)).astype(np.int32)
        case = dict(case, first=first, second=perm[first].astype(np.int32), N=N)
    rng = np.random.default_rng(seed + 9000)
    m = len(case["src"])
    if kw.get("zero"):
        snor = rng.integers(-4, 5, (m, 3)) / 4.0
        snor[np.all(snor == 0, axis=1)] = [0, 1, 0]
    else:
        snor = rng.normal(0, 1, (m, 3))
        snor /= np.linalg.norm(snor, axis=1, keepdims=True)
    case["snor"] = np.ascontiguousarray(snor)
    return case


def gathered(case, first=None, second=None):
    """-> p, q, n_q, n_p of the list"""
    f = case["first"] if first is None else first
    s = case["second"] if second is None else second
    return case["src"][f], case["dst"][s], case["nor"][s], case["snor"][f]


N_FAM = 2001
# explicit lists: every conditioning family of lincases at N = 2 001 (odd: the tail lane runs)
FAMILIES = {fam: [dict(kw, N=N_FAM) for kw in lincases.FAMILIES[fam] if "N" not in kw] for fam in ("t", "W", "unit", "a", "zero", "angle")}
# the count family: tail lane, odd last pair, chunk boundary, many partials
COUNTS = [dict(N=1, chunk=512), dict(N=2, chunk=512), dict(N=511, chunk=512), dict(N=512, chunk=512), dict(N=513, chunk=512),
          dict(N=513, chunk=4096), dict(N=20001, chunk=512), dict(N=20001, chunk=4096)]
# strict-subset lists: n_p through `first`, p from the stream's private copy
SUBSETS = [dict(N=513, M=1500, chunk=512), dict(N=20001, M=30000, chunk=512)]
# searched identity lists: p and n_p from the shared sorted cloud
SEARCHED = [dict(N=513, chunk=512), dict(N=20001)]


def case_name(prefix, kw):
    return prefix + ":" + ",".join("%s=%s" % (k, ("pi" + ("-%g" % (np.pi - v) if v < np.pi else "")) if k == "angle" and v > 3 else "%g" % v) for k, v in kw.items())
