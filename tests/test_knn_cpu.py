"""The neighbour-search contract without a GPU: the numpy reference (tests/knnref.py) against a plain Python loop in k mode, with a bounded
radius and in all mode, and the two entry points exist and reject bad arguments before any device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import knnref
import outlierref
from mvicp import lib as L

ERR_ARG, ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _queries(p, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = p.min(0), p.max(0)
    return np.vstack([rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(20, 3)), p[::17]])


@pytest.mark.parametrize("k,radius", [(1, 0.0), (8, 0.0), (5, 0.08), (64, 0.15), (0, 0.08), (0, 0.3)])
def test_reference_equals_python_loop_on_a_sheet(k, radius):
    p, _, _ = outlierref.sheet_cloud(150, 11)
    q = _queries(p, 1)
    got, want = knnref.knn_search(p, q, k, radius), knnref.knn_search_loop(p, q, k, radius)
    assert knnref.same(got, want)
    assert got["total"] == got["cnt"].sum() > 0
    if radius > 0:   # the radius really bounds: some rows are cut short by it, some hold something
        full = knnref.knn_search(p, q, k if k else 64, 0.0)
        assert (got["cnt"] < full["cnt"]).any() and (got["cnt"] > 0).any()
    if k:
        pad = np.arange(k)[None, :] >= got["cnt"][:, None]
        assert (got["idx"][pad] == -1).all() and np.isposinf(got["d2"][pad]).all() and (got["idx"][~pad] >= 0).all()
    else:
        assert got["off"][-1] == got["total"] == len(got["idx"]) == len(got["d2"])
    assert knnref.same(knnref.knn_search(p, None, k, radius), knnref.knn_search_loop(p, None, k, radius))


@pytest.mark.parametrize("k,radius", [(4, 0.0), (8, 1.0), (0, 1.0), (0, float(np.nextafter(1.0, 2.0))), (0, 1.5)])
def test_reference_equals_python_loop_on_a_shuffled_lattice(k, radius):
    p = knnref.shuffled_lattice(5, 3)
    assert len(p) == 125 and not (np.lexsort(p.T[::-1]) == np.arange(125)).all()
    inner = p[(p <= 3).all(1)]   # (a cell / face centre next to these has all its corners in the lattice)
    q = np.vstack([p[:30], inner[:20] + 0.5, inner[20:40] + [0.5, 0.5, 0.0]])
    got = knnref.knn_search(p, q, k, radius)
    assert knnref.same(got, knnref.knn_search_loop(p, q, k, radius))
    if k == 4 and radius == 0:   # ties cut by k: among equidistant points the lowest indices, ascending
        centre = got["d2"][30:50]
        assert (centre == 0.75).all() and (np.diff(got["idx"][30:50], axis=1) > 0).all()
    if k == 0 and radius == 1.0:   # strict: the neighbours at exactly 1 are out
        assert (got["cnt"][:30] == 1).all()
    if k == 0 and radius > 1.0 and radius < 1.1:
        assert (got["cnt"][:30] >= 4).all() and (got["cnt"][:30] <= 7).all()


def test_reference_degenerate_sizes():
    same_pts = np.tile([[0.25, -0.5, 1.0]], (20, 1))
    r = knnref.knn_search(same_pts, None, 8, 0.0)
    assert (r["idx"] == np.arange(8)).all() and (r["d2"] == 0).all() and not np.signbit(r["d2"]).any()
    r = knnref.knn_search(same_pts[:5], same_pts[:3], 8, 0.0)
    assert (r["cnt"] == 5).all() and (r["idx"][:, 5:] == -1).all() and r["total"] == 15
    r = knnref.knn_search(np.zeros((0, 3)), same_pts[:3], 8, 0.0)
    assert (r["cnt"] == 0).all() and r["idx"].shape == (3, 8) and r["total"] == 0
    r = knnref.knn_search(same_pts, np.zeros((0, 3)), 0, 1.0)
    assert r["off"].tolist() == [0] and r["idx"].shape == (0,)
    with pytest.raises(ValueError):
        knnref.knn_search(same_pts, None, 0, 0.0)


def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mvicp_knn_search", "mvicp_knn_fetch"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)


def test_argument_errors_need_no_gpu(engine_lib):
    search, fetch = engine_lib.mvicp_knn_search, engine_lib.mvicp_knn_fetch
    q = np.zeros((4, 3))
    qp = q.ctypes.data_as(C.c_void_p)
    assert search(None, 0, qp, 4, 8, 0.0) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, 0, None, None, None, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for k in (-1, 65, 1 << 20):
        assert search(ctx, 0, qp, 4, k, 0.0) == ERR_ARG and b"k = " in engine_lib.mvicp_last_error(), k
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert search(ctx, 0, qp, 4, 8, bad) == ERR_ARG and b"radius" in engine_lib.mvicp_last_error(), bad
    for radius in (0.0, -1.0):
        assert search(ctx, 0, qp, 4, 0, radius) == ERR_ARG and b"k = 0" in engine_lib.mvicp_last_error() and b"radius" in engine_lib.mvicp_last_error()
    for m in (-1, 1 << 31, 1 << 40):
        assert search(ctx, 0, qp, m, 8, 0.0) == ERR_ARG and b"m = " in engine_lib.mvicp_last_error(), m
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range), with queries and in self mode
        assert search(ctx, frame, qp, 4, 8, 0.0) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
        assert search(ctx, frame, None, -7, 8, 0.0) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert fake.raw == bytes(1 << 16)
