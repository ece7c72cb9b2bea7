"""The FPFH contract without a GPU: the numpy reference (tests/fpfhref.py) against a plain Python loop, its structure, that it IS the
textbook FPFH (an extended-precision evaluation with atan2 and acos agrees on every pair that is not at a bin edge), and the two entry
points exist and reject bad arguments before any device is needed."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import fpfhref
import knnref
import outlierref
from mvicp import lib as L

ERR_ARG, ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def cloud(name):
    """-> (points, normals, radius, max_nn)"""
    if name == "sheet":
        p, nr, _ = outlierref.sheet_cloud(150, 11)
        return p, nr, 0.15, 16
    p = knnref.shuffled_lattice(5, 3)
    return p, (fpfhref.z_normals(len(p)) if name == "lattice_z" else fpfhref.unit_normals(len(p), 7)), 1.5, 12


# ---- C1
@pytest.mark.parametrize("name", ["sheet", "lattice_z", "lattice_random"])
def test_reference_equals_python_loop(name):
    p, nr, radius, max_nn = cloud(name)
    got = fpfhref.fpfh(p, nr, radius, max_nn)
    assert fpfhref.same(got, fpfhref.fpfh_loop(p, nr, radius, max_nn))
    assert got["pairs"] > 5 * len(p) and (got["used"] == max_nn - 1).any() and (got["used"] < max_nn - 1).any()
    if name == "lattice_z":
        # equal normals along z: a pair along z has e x s = 0; w is orthogonal to s = t, so y = +-0 exactly; a1 == a2 exactly
        assert got["degenerate"] > 0 and got["y_zero"] > 0 and got["swap_ties"] > 0
        assert got["swap_ties"] == got["pairs"] and got["degenerate"] + got["y_zero"] == got["pairs"]
        b = got["bins"][got["valid"]]
        assert (b[:, 0] == 5).all()                     # atan2(0, 1) = 0: the middle bin
    else:
        assert got["degenerate"] == 0


def test_edge_table_is_the_nearest_doubles():
    """cos / sin of -pi + 2 pi k / 11 by their Taylor series in 60-digit decimal arithmetic; float(Decimal) rounds to nearest."""
    import decimal
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        pi = D("3.14159265358979323846264338327950288419716939937510582097494")

        def series(x, first):   # first = 0: cos, 1: sin
            term = x ** first
            total, n = term, first
            while abs(term) > D(10) ** -55:
                term = -term * x * x / ((n + 1) * (n + 2))
                total, n = total + term, n + 2
            return total

        for k, (c, s) in enumerate(fpfhref.EDGES, start=1):
            phi = -pi + 2 * pi * k / 11
            assert c == float(series(phi, 0)) and s == float(series(phi, 1)), k
    assert all(s < 0 for _, s in fpfhref.EDGES[:5]) and all(s > 0 for _, s in fpfhref.EDGES[5:])


def test_theta_bin_on_the_axes_and_edges():
    x = np.array([1.0, 0.0, -1.0, 0.0, 0.0, 1.0, -1.0, -1.0, 1e-300])
    y = np.array([0.0, 1.0, 0.0, -1.0, 0.0, -1e-300, -1e-300, 1e-300, 0.0])
    #            0     pi/2  pi   -pi/2 (0,0) -0+        -pi+     pi-     0
    assert fpfhref._theta_bin(x, y).tolist() == [5, 8, 10, 2, 5, 5, 0, 10, 5]
    assert fpfhref._theta_bin(np.array([1.0]), np.array([-0.0])).tolist() == [5]
    ang = np.linspace(-np.pi, np.pi, 20001)[1:-1]
    want = np.clip(np.floor(11 * (ang + np.pi) / (2 * np.pi)), 0, 10).astype(int)
    got = fpfhref._theta_bin(np.cos(ang), np.sin(ang))
    near_edge = np.abs(11 * (ang + np.pi) / (2 * np.pi) - np.round(11 * (ang + np.pi) / (2 * np.pi))) < 1e-9
    assert (got[~near_edge] == want[~near_edge]).all() and near_edge.sum() <= 1
    assert fpfhref._bin11(np.array([-1.5, -1.0, -1e-17, 0.0, 0.99, 1.0, 7.0])).tolist() == [0, 0, 5, 5, 10, 10, 10]


# ---- C2
def test_structure():
    p, nr, _ = outlierref.sheet_cloud(600, 5)
    p = p.copy()
    dup = [17, 230, 411]
    p[dup] = p[100]                                     # three planted duplicates of point 100 (their normals differ)
    radius, max_nn = 0.05, 6
    knn = knnref.knn_search(p, None, max_nn, radius)
    r = fpfhref.fpfh(p, nr, radius, max_nn, knn)
    m = r["used"]
    spfh = r["spfh"].astype(np.int64).reshape(len(p), 3, 11)
    assert (spfh.sum(2) == m[:, None]).all()
    assert (m == 0).sum() > 0 and (m == max_nn - 1).sum() > 0 and ((m > 0) & (m < max_nn - 1)).sum() > 0
    assert (r["desc"][m == 0] == 0).all() and not np.signbit(r["desc"][m == 0]).any()
    fed = np.array([m[i] > 0 and any(m[j] > 0 for j in knn["idx"][i][r["valid"][i]]) for i in range(len(p))])
    assert fed.sum() > 400
    sums = r["desc"].reshape(len(p), 3, 11).sum(2)
    assert np.abs(sums[fed] - 200.0).max() < 1e-9
    # the duplicates: each of the four sees the other three at d2 == 0 and skips them
    for i in dup + [100]:
        row_d2, row_idx = knn["d2"][i, :knn["cnt"][i]], knn["idx"][i, :knn["cnt"][i]]
        assert (row_d2 == 0).sum() == 4 and sorted(row_idx[:4].tolist()) == sorted(dup + [100])
        assert m[i] == knn["cnt"][i] - 4 and not r["valid"][i, :4].any() and r["valid"][i, 4:knn["cnt"][i]].all()
    assert fpfhref.same(r, fpfhref.fpfh(p, nr, radius, max_nn))
    with pytest.raises(ValueError):
        fpfhref.fpfh(p, nr, 0.0, 16)
    with pytest.raises(ValueError):
        fpfhref.fpfh(p, nr, 0.1, 1)
    empty = fpfhref.fpfh(np.zeros((0, 3)), np.zeros((0, 3)), 0.1, 8)
    assert empty["desc"].shape == (0, 33) and empty["used"].shape == (0,)


# ---- C3
def textbook_pairs(p, nr, knn, valid):
    """PCL's computePairFeatures and its bin rule in extended precision, for the valid pairs -> (bins (P, 3), set_aside (P,))."""
    i, t = np.nonzero(valid)
    j = knn["idx"][i, t]
    P, N = p.astype(LD), nr.astype(LD)
    pi = np.arctan2(LD(0), LD(-1))
    dot = lambda a, b: (a * b).sum(1)
    dp = P[j] - P[i]
    f4 = np.sqrt(dot(dp, dp))
    a1, a2 = dot(N[i], dp), dot(N[j], dp)
    ang1, ang2 = a1 / f4, a2 / f4
    swap = np.arccos(np.minimum(LD(1), np.abs(ang1))) > np.arccos(np.minimum(LD(1), np.abs(ang2)))
    sw = swap[:, None]
    n1, n2, dp = np.where(sw, N[j], N[i]), np.where(sw, N[i], N[j]), np.where(sw, -dp, dp)
    f3 = np.where(swap, -ang2, ang1)
    v = np.cross(dp, n1)
    v = v / np.sqrt(dot(v, v))[:, None]
    w = np.cross(n1, v)
    f2 = dot(v, n2)
    f1 = np.arctan2(dot(w, n2), dot(n1, n2))
    coord = np.stack([11 * (f1 + pi) / (2 * pi), 11 * (f2 + 1) * LD(0.5), 11 * (f3 + 1) * LD(0.5)], 1)
    bins = np.clip(np.floor(coord), 0, 10).astype(np.int64)
    aside = (np.abs(coord - np.round(coord)) < 1e-9).any(1) | (np.abs(np.abs(a1) - np.abs(a2)) < LD(1e-12) * f4)
    return bins, aside


def test_contract_is_fpfh():
    assert np.finfo(LD).eps < 1e-18, "needs an extended-precision long double"
    rng = np.random.Generator(np.random.PCG64(23))
    p = rng.uniform(0.0, 1.0, size=(400, 3))
    nr = fpfhref.unit_normals(400, 29)
    knn = knnref.knn_search(p, None, 32, 0.2)
    r = fpfhref.fpfh(p, nr, 0.2, 32, knn)
    assert r["pairs"] > 4000
    want, aside = textbook_pairs(p, nr, knn, r["valid"])
    assert aside.sum() <= 1e-3 * r["pairs"]
    got = r["bins"][r["valid"]]
    assert (got[~aside] == want[~aside]).all()
    # every bin of every feature occurs: the comparison is not vacuous
    assert all(len(np.unique(got[:, f])) == 11 for f in range(3))
    # and the integer SPFH of the reference is the histogram of exactly these bins
    c = np.zeros((400, 33), dtype=np.int64)
    i, _ = np.nonzero(r["valid"])
    for f in range(3):
        np.add.at(c, (i[~aside], 11 * f + want[~aside, f]), 1)
        np.add.at(c, (i[aside], 11 * f + got[aside, f]), 1)
    assert (c == r["spfh"]).all()


# ---- C4
def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mvicp_fpfh", "mvicp_fpfh_fetch"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)


def test_argument_errors_need_no_gpu(engine_lib):
    fpfh, fetch = engine_lib.mvicp_fpfh, engine_lib.mvicp_fpfh_fetch
    assert fpfh(None, 0, 0.1, 16) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, None) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for max_nn in (-1, 0, 1, 65, 1 << 20):
        assert fpfh(ctx, 0, 0.1, max_nn) == ERR_ARG and b"max_nn = " in engine_lib.mvicp_last_error(), max_nn
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -1.0):
        assert fpfh(ctx, 0, bad, 16) == ERR_ARG and b"radius" in engine_lib.mvicp_last_error(), bad
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range)
        assert fpfh(ctx, frame, 0.1, 16) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert fake.raw == bytes(1 << 16)
