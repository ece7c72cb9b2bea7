"""Per-cloud NN structures built on the GPU (mvicp_set_frame_device) are byte-identical to the host build (mvicp_set_frame) for every
array and scalar mvicp_get_structure exposes, and a registration on device-built clouds is bit-identical to one on host-built clouds."""
import ctypes as C
import os

import numpy as np
import pytest

import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _engines(curve, target, async_build):
    out = []
    for _ in range(2):
        e = mvicp.Engine(0)
        e.set_option("grid_curve", curve)
        e.set_option("grid_target", target)
        e.set_option("async_build", async_build)
        out.append(e)
    return out


def first_difference(eh, ed, frame):
    """(name, byte offset) of the first array in which the two builds of `frame` differ, or None."""
    for name in L.STRUCTURE_NAMES:
        a = eh.get_structure(frame, name).view(np.uint8)
        b = ed.get_structure(frame, name).view(np.uint8)
        if a.size != b.size:
            return name, f"size {a.size} vs {b.size}"
        if not np.array_equal(a, b):
            return name, int(np.flatnonzero(a != b)[0])
    return None


def assert_builds_equal(clouds, normals=None, curve=2, target=5.0, async_build=1):
    eh, ed = _engines(curve, target, async_build)
    try:
        eh.set_frames(clouds, normals)
        ed.set_frames_device([_dev(p) for p in clouds], None if normals is None else [None if n is None else _dev(n) for n in normals])
        for f in range(len(clouds)):
            d = first_difference(eh, ed, f)
            assert d is None, f"frame {f} (n={len(clouds[f])}, grid_curve={curve}, grid_target={target}, async_build={async_build}): first difference in {d[0]} at {d[1]}"
    finally:
        eh.close(); ed.close()


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def small_clouds():
    r = _rng(7)
    cl = {}
    for n in (1, 64, 65, 95, 96, 97, 2047, 2048, 2049, 65537):
        cl[f"n{n}"] = r.normal(size=(n, 3))
    r3 = _rng(8)   # both sides of the boundary between 2 and 3 box levels, and a last node with two boxes (a stream of their own: the clouds below stay what they were)
    for n in (131072, 131073, 133121):
        cl[f"n{n}"] = r3.normal(size=(n, 3))
    base = r.uniform(-1, 1, size=(300, 3))
    cl["duplicates"] = np.vstack([base, base, base[:100]])
    g = np.arange(12, dtype=np.float64)
    cl["lattice"] = np.stack(np.meshgrid(g, g * 0.5, g[:6]), -1).reshape(-1, 3)
    z = np.where(r.random(3000) < 0.5, -0.0, 0.0)
    cl["plane_signed_zero"] = np.column_stack([r.uniform(-1, 1, 3000), r.uniform(-1, 1, 3000), z])
    t = r.uniform(0, 1, 2500)
    cl["line"] = np.column_stack([t, 2 * t, -t])
    cl["one_point"] = np.tile([[0.25, -3.0, 7.5]], (777, 1))
    cl["mm_far"] = -700.0 + 1e-3 * r.uniform(size=(5000, 3))
    # matrix-pipe block scale: 127 / ext exactly on a power of two (ext = 127 / 64), and one ulp either side
    for tag, ext in (("on", 127.0 / 64), ("above", np.nextafter(127.0 / 64, 10.0)), ("below", np.nextafter(127.0 / 64, 0.0))):
        p = r.uniform(-1, 1, size=(1500, 3))
        p[0] = [-ext, 0, 0]
        p[1] = [ext, 0, 0]
        cl[f"scale_{tag}"] = p
    return cl


SMALL = small_clouds()


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("target", [3.0, 5.0, 8.0])
@pytest.mark.parametrize("async_build", [0, 1])
def test_small_and_degenerate_clouds_byte_identical(curve, target, async_build):
    names = sorted(SMALL)
    clouds = [SMALL[k] for k in names]
    normals = [np.roll(c, 1, axis=1) for c in clouds]
    assert_builds_equal(clouds, normals, curve, target, async_build)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_cfg4_view_and_bunny_byte_identical(curve):
    pb = synth.make_problem(2, 200000)
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny18.npz"))
    off = g["row_off"]
    bunny = [g["xyz_e8"][off[k]:off[k + 1]].astype(np.float64) / 1e8 for k in range(0, 18, 3)]
    assert_builds_equal(list(pb["pts"]) + bunny, list(pb["nor"]) + [None] * len(bunny), curve, 5.0, 1)


def test_one_million_points_byte_identical():
    p, n = synth.make_view(3, 64, 1000000)
    assert_builds_equal([p], [n], 2, 5.0, 1)


def test_empty_cloud_matches_host():
    eh, ed = _engines(2, 5.0, 1)
    try:
        eh.set_frames([np.zeros((0, 3)), SMALL["n97"]])
        ed.set_frames_device([_dev(np.zeros((0, 3))), _dev(SMALL["n97"])])
        for e in (eh, ed):
            with pytest.raises(mvicp.MvicpError):
                e.get_structure(0, "spts")
        assert first_difference(eh, ed, 1) is None
    finally:
        eh.close(); ed.close()


def test_registration_and_queries_bit_identical():
    pb = synth.make_problem(8, 50000)
    eh, ed = mvicp.Engine(0), mvicp.Engine(0)
    try:
        eh.set_frames(pb["pts"], pb["nor"])
        ed.set_frames_device([_dev(p) for p in pb["pts"]], [_dev(n) for n in pb["nor"]])
        for e in (eh, ed):
            e.set_graph(pb["src"], pb["dst"])
        Ph, Pd = np.array(pb["init"]), np.array(pb["init"])
        for rnd in range(20):
            ch, wh = eh.correspond(Ph, pb["fixed"], 0.05)
            cd, wd = ed.correspond(Pd, pb["fixed"], 0.05)
            assert np.array_equal(ch, cd), rnd
            assert np.array_equal(np.asarray(wh, np.float32).view(np.uint32), np.asarray(wd, np.float32).view(np.uint32)), rnd
            for k in range(len(pb["src"])):
                for a, b in zip(eh.get_correspondences(k), ed.get_correspondences(k)):
                    assert np.array_equal(a, b), (rnd, k)
            Ph, _ = eh.optimize(Ph, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
            Pd, _ = ed.optimize(Pd, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
            assert np.array_equal(Ph, Pd), rnd
        q = pb["pts"][1][::7] + 0.003
        for m in (L.NN_AUTO, L.NN_BRUTE, L.NN_GRID, L.NN_TILE):
            ih, dh = eh.nn_query(0, q, m)
            idd, dd = ed.nn_query(0, q, m)
            assert np.array_equal(ih, idd) and np.array_equal(dh, dd), m
        nh, kh = eh.recompute_normals(2, 10, want_knn=True)
        nd, kd = ed.recompute_normals(2, 10, want_knn=True)
        assert np.array_equal(nh, nd) and np.array_equal(kh, kd)
    finally:
        eh.close(); ed.close()


def test_tensor_overwritten_after_the_call_changes_nothing():
    p = SMALL["n2049"]
    eh, ed = _engines(2, 5.0, 1)
    try:
        eh.set_frames([p], [p[:, ::-1].copy()])
        t, tn = _dev(p), _dev(p[:, ::-1].copy())
        ed.set_frames_device([t], [tn])
        t.fill_(0)
        tn.fill_(0)
        torch.cuda.synchronize()
        assert first_difference(eh, ed, 0) is None
    finally:
        eh.close(); ed.close()


def test_errors():
    e = mvicp.Engine(0)
    try:
        e.set_frames([np.zeros((5, 3))])
        bad = SMALL["n97"].copy()
        bad[40, 1] = np.nan
        with pytest.raises(mvicp.MvicpError, match="non-finite coordinate in cloud"):
            e.set_frame_device(0, _dev(bad))
        # a host pointer through the C entry itself
        h = np.ascontiguousarray(SMALL["n97"])
        st = e.lib.mvicp_set_frame_device(e.h, 0, h.ctypes.data_as(C.c_void_p), None, len(h))
        assert st == -1, st
        # the library is still usable afterwards (the failed attribute query left no error behind)
        e.set_frame_device(0, _dev(SMALL["n97"]))
        assert e.get_structure(0, "sidx").size == 4 * 97
    finally:
        e.close()


def test_injected_build_failure_is_sticky_until_a_fresh_upload():
    pb = synth.make_problem(3, 3000)
    e = mvicp.Engine(0)
    try:
        e.set_option("async_build", 1)
        e.set_frames_device([_dev(p) for p in pb["pts"]], [_dev(n) for n in pb["nor"]])
        e.get_structure(0, "scalars")   # (waits for those builds: the injected failure must hit the next one)
        e.set_option("fault_inject_build", 1)
        e.set_frame_device(1, _dev(pb["pts"][1]), _dev(pb["nor"][1]))   # the call succeeds; its build fails behind it
        with pytest.raises(mvicp.MvicpError, match="injected structure-build failure"):
            e.set_graph(pb["src"], pb["dst"])
        with pytest.raises(mvicp.MvicpError, match="injected structure-build failure"):
            e.set_graph(pb["src"], pb["dst"])
        e.set_frame_device(1, _dev(pb["pts"][1]), _dev(pb["nor"][1]))
        e.set_graph(pb["src"], pb["dst"])
        counts, _ = e.correspond(pb["init"], pb["fixed"], 0.05)
        assert counts.sum() > 0
    finally:
        e.close()
