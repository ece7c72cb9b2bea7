"""mvicp_segment_plane / mvicp_plane_fetch / mvicp_plane_select / mvicp_plane_fetch_kept on the MI355X: the record, the counts, the flags
and both selections equal the numpy statement of the contract (tests/planeref.py) byte for byte, with host and with device destinations.
What a case must contain (accepted and rejected hypotheses, ties at the top, residuals exactly at tau, a winner that the direction test
changes) is asserted on the reference alone, so no case can pass by rejecting everything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clusterref
import matchref
import mvicp
import outlierref
import planeref as pr
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


_REF = {}


def reference(p, normals, tau, H, seed=0, axis=None, cos_min=0.0, refine=True):
    """The reference result of a call, computed once per (bytes, arguments) and shared; nobody writes into it."""
    key = (p.tobytes(), bool(normals), float(tau), int(H), int(seed), None if axis is None else tuple(float(v) for v in axis), float(cos_min), bool(refine))
    if key not in _REF:
        r = pr.segment(p, np.zeros((len(p), 3)) if normals else None, tau, H, seed, axis, cos_min, refine)
        r["counts"].setflags(write=False); r["flags"].setflags(write=False)
        _REF[key] = r
    return _REF[key]


def check(eng, p, nrm, tau, H, what, seed=0, axis=None, cos_min=0.0, refine=True, frame=0, devices=(False, True)):
    """segment_plane and both selections on the engine's frame against the reference, with host and with device destinations -> the reference"""
    want = reference(p, nrm is not None, tau, H, seed, axis, cos_min, refine)
    for device in devices:
        got = _host(eng.segment_plane(frame, tau, H, seed, axis, cos_min, refine, device=device))
        if not device:
            print(what, "H", H, "refine", refine, {k: got[k] for k in pr.RECORD_INTS})
        assert pr.same(got, want), (what, H, refine, device, {k: (got[k], want[k]) for k in pr.RECORD_INTS + pr.RECORD_VECS},
                                    int((got["counts"] != want["counts"]).sum()), int((got["flags"] != want["flags"]).sum()))
        for inliers in (True, False):
            sel = _host(eng.plane_select(inliers, device=device))
            ws = pr.select(p, nrm, want, inliers)
            assert pr.same_kept(sel, ws), (what, H, inliers, device, sel["kept"], ws["kept"])
    return want


@pytest.mark.parametrize("H", [64, 512])
@pytest.mark.parametrize("refine", [False, True])
def test_noisy_plane(eng, H, refine):
    p, nr, mask = pr.noisy_plane_cloud()
    want = reference(p, True, pr.NOISY_TAU, H, refine=refine)
    assert want["accepted"] == H and want["count"] == (2000 if H == 64 else 2003) and (want["counts"] == want["count"]).sum() == 1
    assert want["refit"] == int(refine) and want["count_refined"] == ((2003 if H == 64 else 2004) if refine else want["count"])
    eng.set_frames([p], [nr])
    check(eng, p, nr, pr.NOISY_TAU, H, "noisy plane", refine=refine)


def test_dyadic_slab(eng):
    """16 x 16 x 3 lattice points: every offset is exact.  tau = pitch / 4: a layer (256 points) is the most a plane can hold, many hypotheses
    reach it, the lowest h wins.  tau = pitch: hypotheses with a point at |r| == tau exactly (the inclusive comparison), ties at 768."""
    p = pr.dyadic_slab()
    quarter, full = reference(p, False, pr.SLAB_PITCH / 4, 512), reference(p, False, pr.SLAB_PITCH, 512)
    top = np.flatnonzero(quarter["counts"] == 256)
    assert (quarter["accepted"], 512 - quarter["accepted"]) == (510, 2) and quarter["count"] == 256 and len(top) == 65 and quarter["best"] == top.min() == 3
    ok, a, m = pr.hypotheses(p, 512, 0)
    exact = (np.abs(pr._residual(m[ok], a[ok], p)) == pr.SLAB_PITCH).any(1)
    assert int(exact.sum()) == 69 and full["count"] == 768 and (full["counts"] == 768).sum() == 21 and full["best"] == np.flatnonzero(full["counts"] == 768).min()
    # seed 0 rejects only its two index collisions; seed 3 has none and rejects two collinear triples of distinct points: nw == 0 exactly
    idx = matchref.sample_indices(3, 512, len(p))
    assert ((idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 2] != idx[:, 0])).all()
    assert reference(p, False, pr.SLAB_PITCH / 4, 512, seed=3)["accepted"] == 510
    eng.set_frames([p], None)
    for refine in (True, False):
        check(eng, p, None, pr.SLAB_PITCH / 4, 512, "slab, tau = pitch / 4", refine=refine)
        check(eng, p, None, pr.SLAB_PITCH, 512, "slab, tau = pitch", refine=refine)
    check(eng, p, None, pr.SLAB_PITCH / 4, 512, "slab, seed 3", seed=3)


def test_rejections(eng):
    line = pr.line_cloud()
    want = reference(line, False, 0.01, 512)
    assert want["accepted"] == 0 and want["best"] == -1 and want["refit"] == 0 and not want["flags"].any() and (want["counts"] == -1).all()
    eng.set_frames([line], None)
    check(eng, line, None, 0.01, 512, "line")
    rest = eng.plane_select(False)
    assert rest["kept"] == len(line) and rest["xyz"].tobytes() == line.tobytes() and eng.plane_select(True)["kept"] == 0
    got = eng.segment_plane(0, 0.01, 512)
    assert got["normal"].tolist() == [0, 0, 0] and got["point"].tolist() == [0, 0, 0] and got["d"] == 0 and got["count"] == 0
    noisy, nr, _ = pr.noisy_plane_cloud()
    twice, twice_n = np.repeat(noisy[:800], 2, axis=0), np.repeat(nr[:800], 2, axis=0)
    want = reference(twice, True, pr.NOISY_TAU, 512)
    assert 0 < want["accepted"] < 512 and want["count"] % 2 == 0 and want["count"] > 1000
    eng.set_frames([twice], [twice_n])
    check(eng, twice, twice_n, pr.NOISY_TAU, 512, "every point twice")
    huge = np.full((100, 3), 1e200) + np.arange(300.0).reshape(100, 3) * 1e185
    want = reference(huge, False, 0.01, 64)
    assert want["accepted"] == 0 and len(np.unique(huge, axis=0)) == 100      # nw overflows: rejected, no error
    eng.set_frames([huge], None)
    check(eng, huge, None, 0.01, 64, "100 points at 1e200")


def test_small_n(eng):
    p = pr.noisy_plane_cloud()[0]
    eng.set_frames([p[:0], p[:1], p[:2], p[:3]], None)
    for n in range(4):
        want = check(eng, p[:n], None, 0.01, 64, "n = %d" % n, frame=n)
        assert want["accepted"] == (21 if n == 3 else 0) and want["n"] == n
    three = reference(p[:3], False, 0.01, 64)
    assert three["count"] == 3 and three["refit"] == 1 and three["best"] == 0
    got = eng.segment_plane(0, 0.01, 64, device=True)
    assert got["flags"].shape == (0,) and got["counts"].shape == (64,) and eng.plane_select(False, device=True)["xyz"].shape == (0, 3)
    one = reference(p[:1], False, 0.01, 64)
    assert pr.select(p[:1], None, one, True)["kept"] == 0 and pr.select(p[:1], None, one, False)["kept"] == 1   # (checked above: frame 1)
    # one workgroup of the compaction with a lane to spare, exactly full, and one point in a second workgroup; the last point is an inlier,
    # so the number kept comes from a kept row in one selection and from a dropped row in the other
    for n, kept in ((255, (249, 6)), (256, (250, 6)), (257, (251, 6))):
        q, nr, _ = outlierref.sheet_cloud(n, 100 + n)
        want = reference(q, True, 0.01, 200, seed=7 + n)
        assert (pr.select(q, nr, want, True)["kept"], pr.select(q, nr, want, False)["kept"]) == kept and want["flags"][-1] == 1
        eng.set_frames([q], [nr])
        check(eng, q, nr, 0.01, 200, "sheet of %d" % n, seed=7 + n)


def test_direction(eng):
    p, floor = pr.floor_wall_cloud()
    free, up = reference(p, False, pr.FLOOR_WALL_TAU, 512), reference(p, False, pr.FLOOR_WALL_TAU, 512, axis=(0.0, 0.0, 2.0), cos_min=0.9)
    assert free["accepted"] == 512 and free["count"] == 2508 and abs(free["normal"][0]) > 0.999 and (free["flags"][~floor] == 1).all()   # the wall wins
    assert up["accepted"] == 75 and up["count"] == 1510 and abs(up["normal"][2]) > 0.999 and (up["flags"][floor] == 1).all()             # the floor wins
    eng.set_frames([p], None)
    check(eng, p, None, pr.FLOOR_WALL_TAU, 512, "floor + wall")
    check(eng, p, None, pr.FLOOR_WALL_TAU, 512, "floor + wall, axis z", axis=(0.0, 0.0, 2.0), cos_min=0.9)
    check(eng, p, None, pr.FLOOR_WALL_TAU, 512, "floor + wall, axis -x, cos 1", axis=(-1.0, 0.0, 0.0), cos_min=1.0, devices=(False,))
    check(eng, p, None, pr.FLOOR_WALL_TAU, 512, "floor + wall, cos 0", axis=(0.3, 0.2, 0.1), cos_min=0.0, devices=(False,))
    assert pr.same(reference(p, False, pr.FLOOR_WALL_TAU, 512, axis=(0.3, 0.2, 0.1), cos_min=0.0), free)   # cos_min = 0 rejects nothing


def test_off_the_origin(eng):
    p, nr, _ = pr.noisy_plane_cloud()
    small, far = np.ascontiguousarray(p * 1e-3 + 1e3), np.ascontiguousarray(p + 4e6)
    ws, wf = reference(small, True, pr.NOISY_TAU * 1e-3, 512), reference(far, True, pr.NOISY_TAU, 512)
    assert ws["count"] == wf["count"] == 2003 and ws["count_refined"] == wf["count_refined"] == 2004 and (ws["q"], wf["q"]) == (31, 21)
    eng.set_frames([small, far], [nr, nr])
    check(eng, small, nr, pr.NOISY_TAU * 1e-3, 512, "scale 1e-3 at 1e3", frame=0)
    check(eng, far, nr, pr.NOISY_TAU, 512, "at 4e6", frame=1)


def _constants():
    txt = open(os.path.join(ROOT, "mv-lm-icp_amd", "csrc", "plane.hip")).read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, txt).group(1)) for k in ("kThreads", "kPointTile", "kWantBlocks")}


def _lattice(n):
    """n points of a 64 x 64 x k lattice at pitch 2^-8 with every fifth-ish point lifted by one pitch: only the bytes matter."""
    i = np.arange(n)
    return np.ascontiguousarray(np.column_stack([i % 64, (i // 64) % 64, i // 4096 + ((i * 7) % 5 == 0)]).astype(np.float64) * 2.0 ** -8)


def test_every_way_through_the_launch_arithmetic(eng):
    K = _constants()
    T, W, B = K["kPointTile"], K["kThreads"], K["kWantBlocks"]
    # the point tiles: one short of a tile, exactly one, one over (= a last chunk of ONE point: with H <= kThreads the chunks are single tiles)
    assert B >= 3
    for n in (T - 1, T, T + 1, 2 * T + 100):
        p = _lattice(n)
        eng.set_frames([p], None)
        assert check(eng, p, None, 2.0 ** -9, 64, "lattice of %d" % n, devices=(False,))["accepted"] > 32
    # chunks of more than one tile: H = 4 kThreads gives kWantBlocks / 4 chunks, so past that many tiles a chunk holds two, and the last
    # chunk of this cloud is one tile and one point: the split ends inside a tile
    gy = B // 4
    n = 2 * T * (gy // 2) + T + 1
    assert -(-n // T) > gy and n % (2 * T) == T + 1
    p = _lattice(n)
    eng.set_frames([p], None)
    assert check(eng, p, None, 2.0 ** -9, 4 * W, "lattice of %d, two-tile chunks" % n, devices=(False,))["accepted"] == 4 * W
    # the accepted hypotheses: 1, and one workgroup of lanes - 1, exactly, + 1 (the number accepted grows by 0 or 1 with H)
    slab = pr.dyadic_slab()
    acc = np.cumsum(pr.hypotheses(slab, 2 * W, 0)[0])
    eng.set_frames([slab, slab[:3]], None)
    for want_acc in (W - 1, W, W + 1):
        H = int(np.flatnonzero(acc == want_acc)[0]) + 1
        assert check(eng, slab, None, pr.SLAB_PITCH, H, "slab, %d accepted" % want_acc, devices=(False,))["accepted"] == want_acc
    one = np.cumsum(pr.hypotheses(slab[:3], 64, 0)[0])
    H = int(np.flatnonzero(one == 1)[0]) + 1
    assert check(eng, slab[:3], None, pr.SLAB_PITCH, H, "three points, one accepted", frame=1, devices=(False,))["accepted"] == 1


def test_bit_rule_at_a_million_inliers(eng):
    """1.1 M points of an exact dyadic plane: c >= 2^20 inliers, so the bit budget drops to b = 20; every sum of the refit is exact."""
    p = pr.dyadic_plane(1_100_000)
    want = reference(p, False, 1e-3, 8)
    assert want["accepted"] == 8 and want["count"] == len(p) >= 1 << 20 and want["b"] == 20 and want["refit"] == 1 and want["count_refined"] == len(p)
    assert abs(want["normal"][2]) == 1.0 and want["normal"][0] == 0 and want["normal"][1] == 0
    eng.set_frames_device([_dev(p)], None)
    check(eng, p, None, 1e-3, 8, "dyadic plane, 1.1 M points", devices=(True,))


def test_pipeline_plane_out_then_cluster(eng):
    tt, part = pr.tabletop_cloud()
    one = clusterref.cluster(tt, None, pr.TABLE_RADIUS, pr.TABLE_MIN_PTS)
    assert one["stats"]["clusters"] == 1 and one["stats"]["noise"] == 0      # the floor joins both boxes into ONE cluster
    eng.set_frames([tt], None)
    assert clusterref.same(eng.cluster(0, pr.TABLE_RADIUS, pr.TABLE_MIN_PTS), one)
    want = check(eng, tt, None, pr.TABLE_TAU, 256, "tabletop")
    assert (want["flags"][part == 0] == 1).all() and not want["flags"][part != 0].any()
    rest = eng.plane_select(False, device=True)
    eng.set_frames_device([rest["xyz"]], None)
    idx = rest["idx"].cpu().numpy()
    two = clusterref.cluster(tt[idx], None, pr.TABLE_RADIUS, pr.TABLE_MIN_PTS)
    got = eng.cluster(0, pr.TABLE_RADIUS, pr.TABLE_MIN_PTS)
    assert clusterref.same(got, two) and got["stats"]["clusters"] == 2 and got["stats"]["noise"] == 0
    assert [set(part[idx][got["label"] == k].tolist()) for k in (0, 1)] in ([{1}, {2}], [{2}, {1}])   # the two clusters ARE the two boxes
    # repeated extraction is the caller's loop: the rest of floor + wall holds the other plane
    fw, floor = pr.floor_wall_cloud()
    eng.set_frames([fw], None)
    first = check(eng, fw, None, pr.FLOOR_WALL_TAU, 512, "floor + wall, first plane", devices=(False,))
    rest = eng.plane_select(False, device=True)
    left = np.ascontiguousarray(fw[rest["idx"].cpu().numpy()])
    eng.set_frames_device([rest["xyz"]], None)
    second = check(eng, left, None, pr.FLOOR_WALL_TAU, 512, "floor + wall, second plane")
    assert abs(first["normal"][0]) > 0.999 and abs(second["normal"][2]) > 0.999 and second["count_refined"] >= 1490
    assert len(left) == len(fw) - first["count_refined"]


def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_planes):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_planes:
                e.segment_plane(2, 0.01, 128)   # before the graph exists
                e.plane_select(False)
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_planes:
                    e.segment_plane(r, 0.02, 256, seed=r)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_planes:
                    e.segment_plane(3 - r, 0.005, 64, axis=(0.0, 0.0, 1.0), cos_min=0.5, refine=(r != 1), device=(r == 2))
                    e.plane_select(r == 0, device=(r == 2))
                triples, offsets = e.map_correspondences()
                blocks = e.linearize(poses, True, True)
                if with_planes:
                    e.plane_select(True)
                poses, sm = e.optimize(poses, pb["fixed"])
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_state_and_errors(eng):
    p, nr, _ = pr.noisy_plane_cloud()
    p, nr = np.ascontiguousarray(p[:900]), np.ascontiguousarray(nr[:900])
    want = pr.segment(p, None, pr.NOISY_TAU, 96, 5)
    assert want["accepted"] == 96 and want["refit"] == 1 and 0 < want["count_refined"] < len(p)
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        seg, fetch, select, kept = lib.mvicp_segment_plane, lib.mvicp_plane_fetch, lib.mvicp_plane_select, lib.mvicp_plane_fetch_kept
        R = mvicp.lib.PlaneResult()
        assert fetch(h, 10, None, 10, None) == ERR_STATE and select(h, 1) == ERR_STATE and kept(h, 10, None, None, None) == ERR_STATE   # before any call
        assert seg(h, 0, 96, 5, pr.NOISY_TAU, None, 0.0, 1, C.byref(R)) == ERR_ARG                     # frames not declared: out of range
        assert lib.mvicp_set_num_frames(h, 3) == 0
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.mvicp_set_frame(h, 0, dp(p), None, len(p)) == 0
        assert seg(h, 1, 96, 5, pr.NOISY_TAU, None, 0.0, 1, C.byref(R)) == ERR_STATE and b"never uploaded" in lib.mvicp_last_error()
        assert seg(h, 0, 96, 5, pr.NOISY_TAU, None, 0.0, 1, C.byref(R)) == 0
        got = R.as_dict()
        assert all(int(got[k]) == int(want[k]) for k in pr.RECORD_INTS) and all(np.asarray(got[k]).tobytes() == np.asarray(want[k], dtype=np.float64).tobytes() for k in pr.RECORD_VECS)
        counts, flags = np.zeros(96, np.int32), np.zeros(len(p), np.uint8)

        def result_is_still_there():
            assert fetch(h, 96, vp(counts), len(p), vp(flags)) == 0
            assert counts.tobytes() == want["counts"].tobytes() and flags.tobytes() == want["flags"].tobytes()

        result_is_still_there()
        assert kept(h, len(p), None, None, None) == ERR_STATE and b"select" in lib.mvicp_last_error()   # a result, but no selection yet
        # refused calls keep the earlier result: every argument error is decided before the context is touched
        zero, nan_axis, z = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(0.0, float("nan"), 1.0), (C.c_double * 3)(0.0, 0.0, 1.0)
        for args in ((0, 0, pr.NOISY_TAU, None, 0.0), (0, (1 << 24) + 1, pr.NOISY_TAU, None, 0.0), (0, 96, float("nan"), None, 0.0), (0, 96, 0.0, None, 0.0),
                     (0, 96, -1.0, None, 0.0), (0, 96, float("inf"), None, 0.0), (0, 96, 0.01, zero, 0.5), (0, 96, 0.01, nan_axis, 0.5), (0, 96, 0.01, z, 1.5),
                     (0, 96, 0.01, z, -0.5), (3, 96, 0.01, None, 0.0), (-1, 96, 0.01, None, 0.0)):
            assert seg(h, args[0], args[1], 5, args[2], args[3], args[4], 1, C.byref(R)) == ERR_ARG, args[:3]
            result_is_still_there()
        assert seg(h, 0, 96, 5, pr.NOISY_TAU, None, 0.0, 1, None) == ERR_ARG
        result_is_still_there()
        ws = pr.select(p, None, want, False)
        assert 0 < ws["kept"] < len(p) and select(h, 0) == ws["kept"]
        xyz, idx = np.zeros((len(p), 3)), np.zeros(len(p), np.int32)
        assert kept(h, ws["kept"] - 1, vp(xyz), None, None) == ERR_ARG                                   # cap < kept
        assert fetch(h, 95, vp(counts), 0, None) == ERR_ARG and fetch(h, 0, None, len(p) - 1, vp(flags)) == ERR_ARG
        assert kept(h, ws["kept"], vp(xyz), vp(xyz), None) == ERR_STATE and b"normals" in lib.mvicp_last_error()   # nrm of a frame without normals
        assert kept(h, ws["kept"], vp(xyz), None, vp(idx)) == 0
        assert xyz[:ws["kept"]].tobytes() == ws["xyz"].tobytes() and idx[:ws["kept"]].tobytes() == ws["idx"].tobytes()
        # an upload to another slot leaves the result, an upload to the segmented frame ends it; so does mvicp_set_num_frames
        assert lib.mvicp_set_frame(h, 1, dp(p), dp(nr), len(p)) == 0
        result_is_still_there()
        assert lib.mvicp_set_frame(h, 0, dp(p), None, len(p)) == 0
        assert fetch(h, 96, vp(counts), 0, None) == ERR_STATE and select(h, 1) == ERR_STATE and kept(h, len(p), None, None, None) == ERR_STATE
        assert seg(h, 1, 96, 5, pr.NOISY_TAU, None, 0.0, 1, C.byref(R)) == 0 and R.has_normals == 1 and select(h, 1) == want["count_refined"]
        nrm = np.zeros((len(p), 3))
        assert kept(h, len(p), None, vp(nrm), None) == 0 and nrm[:want["count_refined"]].tobytes() == nr[want["flags"] == 1].tobytes()
        assert lib.mvicp_set_num_frames(h, 1) == 0 and fetch(h, 1 << 20, None, 1 << 20, None) == ERR_STATE
    finally:
        fresh.close()
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        eng.segment_plane(0, float("nan"))
