"""The outlier-filter contract without a GPU: the numpy reference (tests/outlierref.py) against a plain Python loop, the host function
mvicp_outlier_threshold against the rule in Python integers, and the three entry points exist and reject bad arguments before any
device is needed."""
import ctypes as C
import math

import numpy as np
import pytest

import mvicp
import outlierref
from mvicp import lib as L

ERR_ARG, ERR_STATE = -1, -3


@pytest.mark.parametrize("k,std_ratio,radius", [(1, 2.0, 0.0), (4, 1.0, 0.25), (8, 0.0, 0.0), (3, -1.0, 0.2), (5, -1.0, 0.0)])
def test_reference_equals_python_loop(k, std_ratio, radius):
    p, nr, planted = outlierref.sheet_cloud(150, 11)
    got, want = outlierref.outlier_filter(p, nr, k, std_ratio, radius), outlierref.outlier_filter_loop(p, nr, k, std_ratio, radius)
    assert outlierref.same(got, want)
    assert got["kd2"].min() > 0 and (got["mdist"] > 0).all()
    if std_ratio < 0 and radius <= 0:
        assert got["stats"]["kept"] == 150 and got["stats"]["q_exp"] == 0 and got["stats"]["s1"] == 0
    else:
        assert 0 < got["stats"]["kept"] < 150 and not set(planted) <= set(got["idx"].tolist())
    assert outlierref.same(outlierref.outlier_filter(p, None, k, std_ratio, radius), outlierref.outlier_filter_loop(p, None, k, std_ratio, radius))


def test_reference_on_ties_and_identical_points():
    p, nr = outlierref.lattice_cloud()
    assert len(p) == 293 and outlierref.tie_count(p, 8) >= 1
    sub = np.vstack([p[:40], p[-5:]])
    assert outlierref.same(outlierref.outlier_filter(sub, None, 8, 2.0, 0.0), outlierref.outlier_filter_loop(sub, None, 8, 2.0, 0.0))
    same_pts = np.tile([[0.25, -0.5, 1.0]], (20, 1))
    r = outlierref.outlier_filter(same_pts, None, 8, 2.0, 0.01)
    assert r["stats"]["kept"] == 20 and r["stats"]["q_exp"] == 0 and (r["kd2"] == 0).all() and not np.signbit(r["kd2"]).any()
    assert outlierref.outlier_filter(np.zeros((0, 3)), None, 8, 2.0, 0.0)["stats"]["kept"] == 0
    with pytest.raises(ValueError):
        outlierref.outlier_filter(same_pts[:8], None, 8, 2.0, 0.0)   # 0 < n <= k


def _sets():
    """(n, M) sets of the threshold test: random ones of every size class, sums whose n S2 - S1^2 exceeds 2^64, all M equal, two values."""
    rng = np.random.Generator(np.random.PCG64(2024))
    out = []
    for n in (2, 3, 7, 64, 1000, 20000):
        for top in (1 << 31, 1 << 20, 5):
            out.append([int(v) for v in rng.integers(0, top, size=n)])
    out.append([int(v) for v in rng.integers(1 << 30, 1 << 31, size=50000)])   # n S2 - S1^2 ~ 2^89
    out.append([(1 << 31) - 1] * 999 + [0])
    out.append([1234567] * 300)                                                   # var = 0
    out.append([(1 << 31) - 1] * 2)
    out.append([0, 0, 0, 1])
    return out


def test_threshold_equals_python_rule(engine_lib):
    big = 0
    for M in _sets():
        n, s1, s2 = len(M), sum(M), sum(m * m for m in M)
        big += (n * s2 - s1 * s1) >> 64 > 0
        for ratio in (2.0, 0.0, 1.0 / 3.0, -0.75, 10.0):
            want = outlierref.threshold(n, s1, s2, ratio)
            got = mvicp.outlier_threshold(n, s1, s2, ratio)
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (n, ratio, got, want)
        if len(set(M)) == 1:
            assert n * s2 - s1 * s1 == 0 and mvicp.outlier_threshold(n, s1, s2, 2.0) == float(M[0])
    assert big >= 5
    # synthetic sums far beyond what a cloud can give: the 128-bit difference converts like Python's float(int), halfway cases included
    rng = np.random.Generator(np.random.PCG64(7))
    for bits in list(range(60, 127, 3)) + [126]:
        for halfway in (False, True):
            v = (1 << (bits - 1)) | int(rng.integers(0, 1 << 62)) % (1 << (bits - 1))   # a `bits`-bit integer
            if halfway:
                sh = bits - 53
                v = ((v >> sh) << sh) | (1 << (sh - 1))   # exactly between two doubles
            # n S2 - S1^2 = v with n = 2 and S1 = 0 or 1: S2 = (v + S1^2) / 2 needs the same parity
            s1 = v & 1
            s2 = (v + s1) // 2
            assert 2 * s2 - s1 * s1 == v and v.bit_length() == bits
            want = outlierref.threshold(2, s1, s2, 1.0)
            assert np.float64(mvicp.outlier_threshold(2, s1, s2, 1.0)).tobytes() == np.float64(want).tobytes(), (bits, halfway)


def test_threshold_argument_errors(engine_lib):
    T = C.c_double(0.0)
    f = engine_lib.mvicp_outlier_threshold
    assert f(1, 5, 0, 25, 2.0, C.byref(T)) == ERR_ARG                      # n < 2
    assert f(2, 5, 0, 25, 2.0, None) == ERR_ARG
    assert f(2, 5, 0, 25, float("nan"), C.byref(T)) == ERR_ARG
    assert f(2, 5, 0, 25, float("inf"), C.byref(T)) == ERR_ARG
    assert f(2, 10, 0, 25, 2.0, C.byref(T)) == ERR_ARG                     # S1^2 > n S2: not the sums of one set
    assert f(4, 0, 1 << 63, 0, 2.0, C.byref(T)) == ERR_ARG                 # n S2 does not fit 128 bits
    assert f(2, 10, 0, 50, 2.0, C.byref(T)) == 0 and T.value == 5.0


def test_symbols_and_argument_errors_need_no_gpu(engine_lib):
    for name in ("mvicp_outlier_filter", "mvicp_outlier_fetch", "mvicp_outlier_threshold"):
        assert name in L.SYMBOLS and hasattr(engine_lib, name)
    filt, fetch = engine_lib.mvicp_outlier_filter, engine_lib.mvicp_outlier_fetch
    assert filt(None, 0, 8, 2.0, 0.0, None) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, None, None, 0, None, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    S = L.OutlierStats()
    for k in (0, -1, 33, 1 << 20):
        assert filt(ctx, 0, k, 2.0, 0.0, C.byref(S)) == ERR_ARG and b"k = " in engine_lib.mvicp_last_error(), k
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert filt(ctx, 0, 8, bad, 0.0, None) == ERR_ARG and b"std_ratio" in engine_lib.mvicp_last_error(), bad
        assert filt(ctx, 0, 8, 2.0, bad, None) == ERR_ARG and b"radius" in engine_lib.mvicp_last_error(), bad
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range)
        assert filt(ctx, frame, 8, 2.0, 0.0, None) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert fake.raw == bytes(1 << 16)
    assert math.isfinite(mvicp.outlier_threshold(3, 6, 14, 2.0))
