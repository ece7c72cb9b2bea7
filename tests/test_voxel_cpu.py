"""The voxel-grid contract without a GPU: the numpy reference (tests/voxelref.py) against a plain Python loop, the lattice case really
tells floor(w / h) from floor(w * (1 / h)), and the two entry points exist and reject bad arguments before any device is needed."""
import ctypes as C

import numpy as np
import pytest

import voxelref
from mvicp import lib as L
from mvicp import synth

ERR_ARG = -1


def test_reference_equals_python_loop():
    pts, nor, h = voxelref.small_case()
    assert len(pts) == 200 and np.signbit(pts[pts == 0.0]).any() and (pts[:, 0] < 0).any() and (pts[:, 0] > 0).any()
    got, want = voxelref.voxel_grid([pts], [nor], h), voxelref.voxel_grid_loop([pts], [nor], h)
    assert voxelref.same(got, want)
    assert (got["cnt"] == 1).any() and (got["cnt"] > 1).any() and got["cnt"].sum() == 200
    # without normals, and as two frames at poses (a second order of summation)
    assert voxelref.same(voxelref.voxel_grid([pts], None, h), voxelref.voxel_grid_loop([pts], None, h))
    P = synth.make_poses(2)["init"]
    for frames in (None, [1, 0]):
        a = voxelref.voxel_grid([pts[:120], pts[120:]], [nor[:120], nor[120:]], h, frames, P)
        b = voxelref.voxel_grid_loop([pts[:120], pts[120:]], [nor[:120], nor[120:]], h, frames, P)
        assert voxelref.same(a, b), frames


def test_lattice_case_discriminates_division_from_reciprocal():
    pts, nor, h = voxelref.lattice_case()
    k = np.arange(-2000, 2000)
    assert int((np.floor((k * h) / h) != k).sum()) == 303     # the quotient is the contract, not k
    div, rec = voxelref.cells(pts, h), voxelref.cells(pts, h, reciprocal=True)
    assert (div != rec).any(axis=1).sum() >= 1
    ref = voxelref.voxel_grid([pts], [nor], h)
    assert voxelref.same(ref, voxelref.voxel_grid_loop([pts], [nor], h))
    assert (np.abs(ref["nrm"]).sum(axis=1) == 0.0).any()       # cancelled normal sums give (0,0,0) rows
    assert np.signbit(pts[:, 1]).any() and not np.signbit(ref["xyz"][:, 1]).any()   # +0.0 + -0.0 = +0.0


def test_reference_range_errors():
    p = np.array([[0.5, 0.5, 0.5], [-0.5, 0.25, 0.125]])
    with pytest.raises(ValueError):
        voxelref.voxel_grid([p], None, 1e-12)          # quotient >= 2^31
    with pytest.raises(ValueError):
        voxelref.voxel_grid([p * 1e3], None, 1e-6)     # 10^9 cells per axis: d_x d_y d_z >= 2^62
    assert voxelref.voxel_grid([np.zeros((0, 3))], None, 0.1)["cnt"].shape == (0,)


def test_symbols_and_argument_errors_need_no_gpu(engine_lib):
    assert "mvicp_voxel_grid" in L.SYMBOLS and "mvicp_voxel_fetch" in L.SYMBOLS
    grid, fetch = engine_lib.mvicp_voxel_grid, engine_lib.mvicp_voxel_fetch
    hn = C.c_int(7)
    assert grid(None, 0, None, None, 0.01, C.byref(hn)) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, None, None) == ERR_ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert grid(None, 0, None, None, bad, None) == ERR_ARG, bad
    assert grid(None, -1, None, None, 0.01, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert grid(ctx, 0, None, None, bad, None) == ERR_ARG and b"voxel" in engine_lib.mvicp_last_error(), bad
    assert grid(ctx, -1, None, None, 0.01, None) == ERR_ARG and b"n_sel" in engine_lib.mvicp_last_error()
    assert fake.raw == bytes(1 << 16)
