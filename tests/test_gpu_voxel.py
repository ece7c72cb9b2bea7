"""mvicp_voxel_grid / mvicp_voxel_fetch on the MI355X: every result equals the numpy statement of the contract (tests/voxelref.py) byte for
byte — values, counts and row order."""
import ctypes as C

import numpy as np
import pytest

import mvicp
import pathcases
import voxelref
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _host(r):
    return {k: (None if v is None else (v.cpu().numpy() if isinstance(v, torch.Tensor) else v)) for k, v in r.items()}


def assert_same(got, want, what):
    got = _host(got)
    assert (got["nrm"] is None) == (want["nrm"] is None), what
    assert got["cnt"].dtype == np.int32 and got["cnt"].shape == want["cnt"].shape, (what, got["cnt"].shape, want["cnt"].shape)
    assert got["cnt"].tobytes() == want["cnt"].tobytes(), (what, "cnt")
    for k in ("xyz", "nrm"):
        if want[k] is not None:
            assert got[k].dtype == np.float64 and got[k].shape == want[k].shape, (what, k)
            bad = np.argwhere(np.ascontiguousarray(got[k]).view(np.uint64) != np.ascontiguousarray(want[k]).view(np.uint64))
            assert got[k].tobytes() == want[k].tobytes(), (what, k, len(bad), bad[:4].tolist())


def box_cloud(n, seed):
    """n random points in a box that straddles the origin ([-0.4, 0.6]^3), with unit normals."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = rng.uniform(-0.4, 0.6, size=(n, 3))
    nr = rng.normal(size=(n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return p, nr


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 5000])
@pytest.mark.parametrize("mode", ["one_per_voxel", "eight_per_voxel", "octants", "one_voxel"])
def test_single_frame_without_poses(eng, n, mode):
    """(a) nearly every voxel one point, (b) about 8 per voxel, (c) a voxel far larger than the cloud.  A box that straddles the origin spans
    the eight cells that meet there ("octants": runs of n / 8); the same cloud moved into the positive octant lies in ONE voxel (a
    sequential run of all n points)."""
    p, nr = box_cloud(n, 100 + n)
    h = {"one_per_voxel": 1e-4, "eight_per_voxel": (8.0 / n) ** (1.0 / 3.0), "octants": 4.0, "one_voxel": 4.0}[mode]
    if mode == "one_voxel":
        p = p + 1.0
    eng.set_frames([p], [nr])
    want = voxelref.voxel_grid([p], [nr], h)
    if mode == "one_voxel":
        assert list(want["cnt"]) == [n]
    if mode == "one_per_voxel":
        assert len(want["cnt"]) >= 0.99 * n
    if mode == "eight_per_voxel" and n == 5000:
        assert 4.0 <= n / len(want["cnt"]) <= 12.0
    for permute in (1, 0):
        eng.set_option("voxel_permute", permute)
        assert_same(eng.voxel_grid(h), want, (n, mode, permute))
    eng.set_option("voxel_permute", 1)


def test_lattice_and_signed_zeros(eng):
    p, nr, h = voxelref.lattice_case()
    assert (voxelref.cells(p, h) != voxelref.cells(p, h, reciprocal=True)).any()
    eng.set_frames([p], [nr])
    want = voxelref.voxel_grid([p], [nr], h)
    assert (np.abs(want["nrm"]).sum(axis=1) == 0.0).any()
    for permute in (1, 0):
        eng.set_option("voxel_permute", permute)
        assert_same(eng.voxel_grid(h), want, ("lattice", permute))
    eng.set_option("voxel_permute", 1)


def test_many_runs_cross_block_boundaries(eng):
    p, nr = box_cloud(70000, 7)
    h = (1.0 / 20000.0) ** (1.0 / 3.0)
    want = voxelref.voxel_grid([p], [nr], h)
    assert 15000 <= len(want["cnt"]) <= 25000
    eng.set_frames([p], [nr])
    for permute in (1, 0):
        eng.set_option("voxel_permute", permute)
        assert_same(eng.voxel_grid(h), want, ("many runs", permute))
    eng.set_option("voxel_permute", 1)


def test_several_frames_with_poses(eng):
    pb = synth.make_problem(3, 3000)
    h = 0.01
    eng.set_frames(pb["pts"], pb["nor"])
    ref = {}
    for frames in (None, [2, 0], [0, 2], [1]):
        want = ref[str(frames)] = voxelref.voxel_grid(pb["pts"], pb["nor"], h, frames, pb["init"])
        for permute in (1, 0):
            eng.set_option("voxel_permute", permute)
            assert_same(eng.voxel_grid(h, frames, pb["init"]), want, (frames, permute))
    eng.set_option("voxel_permute", 1)
    # the order of summation is really under test: the two orders of the same frames differ in some bytes
    a, b = ref["[2, 0]"], ref["[0, 2]"]
    assert a["cnt"].tobytes() == b["cnt"].tobytes() and (a["cnt"] > 1).any()
    assert a["xyz"].tobytes() != b["xyz"].tobytes() or a["nrm"].tobytes() != b["nrm"].tobytes()
    # poses given but frames stored as they are: NULL poses is "no arithmetic", not the identity's
    assert_same(eng.voxel_grid(h, [1]), voxelref.voxel_grid(pb["pts"], pb["nor"], h, [1]), "stored")


@pytest.mark.parametrize("h", pathcases.V1_VOXELS)
def test_wide_keys(eng, h):
    """V1: two clusters 1000 (then 1200) apart on every axis at a millimetre voxel: a million cells per axis, negative and positive, and a
    sort over 60 (then 61) key bits, the widest below the refusal; further apart the cell count passes 2^62, which is refused and leaves
    the context usable."""
    for shift in (pathcases.V1_SHIFT, pathcases.V1_SHIFT_WIDER):
        bits, want = pathcases.check_voxel_v1(shift, h)
        p, nr = pathcases.voxel_two_clusters(shift)
        eng.set_frames([p], [nr])
        for permute in (1, 0):
            eng.set_option("voxel_permute", permute)
            assert_same(eng.voxel_grid(h), want, ("wide keys", shift, h, bits, permute))
        eng.set_option("voxel_permute", 1)
    p, nr = pathcases.voxel_two_clusters(pathcases.V1_SHIFT_REFUSED)
    assert pathcases.voxel_key_bits(p, h)[1] >= 2 ** 62
    with pytest.raises(ValueError, match="too small for the extent"):
        voxelref.voxel_grid([p], [nr], h)
    eng.set_frames([p], [nr])
    for permute in (1, 0):
        eng.set_option("voxel_permute", permute)
        with pytest.raises(mvicp.MvicpError, match="too small for the extent"):
            eng.voxel_grid(h)
        assert_same(eng.voxel_grid(0.04), voxelref.voxel_grid([p], [nr], 0.04), ("after the refusal", h, permute))
    eng.set_option("voxel_permute", 1)


def test_georeferenced_and_fused(eng):
    """V2: three frames with poses at UTM coordinates, fused at a centimetre voxel (quotients above 4e8); a millimetre voxel there passes
    2^31 cells from the origin, which is an argument error that leaves the context usable."""
    want = pathcases.check_voxel_v2()
    pts, nor, poses = pathcases.voxel_v2_problem()
    eng.set_frames(pts, nor)
    for permute in (1, 0):
        eng.set_option("voxel_permute", permute)
        assert_same(eng.voxel_grid(pathcases.V2_VOXEL, None, poses), want, ("utm", permute))
        with pytest.raises(mvicp.MvicpError, match="status -1"):
            eng.voxel_grid(pathcases.V2_VOXEL_REFUSED, None, poses)
        assert b"2^31" in eng.lib.mvicp_last_error()
        assert_same(eng.voxel_grid(pathcases.V2_VOXEL, None, poses), want, ("utm, after the refusal", permute))
    eng.set_option("voxel_permute", 1)


def test_normals_empty_frames_and_empty_selections(eng):
    pb = synth.make_problem(3, 1000)
    h = 0.01
    empty = np.zeros((0, 3))
    eng.set_frames(pb["pts"], None)
    got = eng.voxel_grid(h, poses=pb["gt"])
    assert got["nrm"] is None
    assert_same(got, voxelref.voxel_grid(pb["pts"], None, h, None, pb["gt"]), "no normals")
    m = len(got["cnt"])
    buf = np.zeros((m, 3))
    st = eng.lib.mvicp_voxel_fetch(eng.h, m, None, buf.ctypes.data_as(C.c_void_p), None)
    assert st == ERR_STATE and b"normals" in eng.lib.mvicp_last_error()
    # mixed: frame 1 without normals; an empty frame (with or without normals) contributes nothing and does not decide has_normals
    pts = [pb["pts"][0], pb["pts"][1], empty, pb["pts"][2]]
    nor = [pb["nor"][0], None, None, pb["nor"][2]]
    P = np.array([pb["gt"][0], pb["gt"][1], np.eye(4), pb["gt"][2]])
    eng.set_frames(pts, nor)
    got = eng.voxel_grid(h, None, P)
    assert got["nrm"] is None
    assert_same(got, voxelref.voxel_grid(pts, nor, h, None, P), "mixed")
    got = eng.voxel_grid(h, [3, 2, 0], P)
    assert got["nrm"] is not None
    assert_same(got, voxelref.voxel_grid(pts, nor, h, [3, 2, 0], P), "empty frame inside")
    assert_same(got, voxelref.voxel_grid(pts, nor, h, [3, 0], P), "empty frame contributes nothing")
    for frames in ([2], []):
        got = eng.voxel_grid(h, frames, P)
        assert len(got["cnt"]) == 0 and got["xyz"].shape == (0, 3), frames
        got = eng.voxel_grid(h, frames, P, device=True)
        assert got["xyz"].shape == (0, 3) and got["cnt"].shape == (0,), frames


def test_device_upload_and_device_fetch(eng):
    pb = synth.make_problem(3, 3000)
    h = 0.008
    want = voxelref.voxel_grid(pb["pts"], pb["nor"], h, None, pb["init"])
    eng.set_frames_device([_dev(p) for p in pb["pts"]], [_dev(n) for n in pb["nor"]])
    got = eng.voxel_grid(h, None, pb["init"])
    assert_same(got, want, "device upload")
    dev = eng.voxel_grid(h, None, pb["init"], device=True)
    assert all(isinstance(dev[k], torch.Tensor) and dev[k].is_cuda for k in ("xyz", "nrm", "cnt"))
    assert_same(dev, want, "device fetch")
    # the device result goes straight into another engine; its structures equal those of the numpy result uploaded from the host
    a, b = mvicp.Engine(0), mvicp.Engine(0)
    try:
        a.set_frames_device([dev["xyz"]], [dev["nrm"]])
        b.set_frames([got["xyz"]], [got["nrm"]])
        for name in ("spts", "snor", "sidx"):
            assert a.get_structure(0, name).tobytes() == b.get_structure(0, name).tobytes(), name
    finally:
        a.close(); b.close()


def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_grid):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"]); e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_grid:
                    e.voxel_grid(0.01, None if r % 2 == 0 else [3, 1], poses)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_grid:
                    e.voxel_grid(0.02 if r else 0.005, [r], None)
                poses, sm = e.optimize(poses, pb["fixed"])
                out.append((counts.tobytes(), weights.tobytes(), poses.tobytes(), sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_errors(eng):
    rng = np.random.Generator(np.random.PCG64(3))
    p = rng.uniform(-0.5, 0.5, size=(500, 3))
    fresh = mvicp.Engine(0)
    try:
        assert fresh.lib.mvicp_voxel_fetch(fresh.h, 10, None, None, None) == ERR_STATE          # a fetch before any grid call
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 0, None, None, 0.1, None) == ERR_STATE       # frames not declared
        fresh.set_frames([p, p + 0.25], None)
        assert fresh.lib.mvicp_set_num_frames(fresh.h, 3) == 0
        q = np.ascontiguousarray(p)
        assert fresh.lib.mvicp_set_frame(fresh.h, 0, q.ctypes.data_as(C.POINTER(C.c_double)), None, len(q)) == 0
        sel = np.array([0, 0], dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 0, None, None, 0.1, None) == ERR_STATE       # "all frames", frames 1 and 2 never uploaded
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 1, ip(sel[1:] + 2), None, 0.1, None) == ERR_STATE
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 1, ip(sel), None, 0.1, None) > 0            # frame 0 alone is fine
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 2, ip(sel), None, 0.1, None) == ERR_ARG      # listed twice
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 1, ip(sel + 3), None, 0.1, None) == ERR_ARG  # out of range
        assert fresh.lib.mvicp_voxel_grid(fresh.h, 1, ip(sel - 1), None, 0.1, None) == ERR_ARG
    finally:
        fresh.close()
    eng.set_frames([p], None)
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        eng.voxel_grid(1e-12)                                   # quotient >= 2^31
    with pytest.raises(mvicp.MvicpError, match="status -3"):   # a failed grid call leaves no result behind
        L._check(eng.lib, eng.lib.mvicp_voxel_fetch(eng.h, 1 << 20, None, None, None))
    eng.set_frames([p * 1e3], None)
    with pytest.raises(mvicp.MvicpError, match="too small for the extent"):
        eng.voxel_grid(1e-6)                                    # 10^9 cells per axis
    eng.set_frames([p], None)
    P = np.eye(4)[None].copy()
    P[0, 1, 2] = np.nan
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        eng.voxel_grid(0.1, None, P)
    m = len(eng.voxel_grid(0.1)["cnt"])
    assert m > 1
    buf = np.zeros((m, 3))
    assert eng.lib.mvicp_voxel_fetch(eng.h, m - 1, buf.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG      # cap < m
    assert eng.lib.mvicp_voxel_fetch(eng.h, m, buf.ctypes.data_as(C.c_void_p), None, None) == 0
    assert buf.tobytes() == voxelref.voxel_grid([p], None, 0.1)["xyz"].tobytes()
