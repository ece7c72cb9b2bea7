"""mvicp_iss_keypoints / mvicp_iss_fetch on the MI355X: idx, xyz, saliency, cnt_salient and cnt_nms equal the numpy statement of the
contract (tests/issref.py) byte for byte; no tolerance anywhere.  What the cases contain is asserted on the reference alone in
tests/test_iss_cpu.py; which way out of the traversal a point takes is derived here from the grid the library built."""
import ctypes as C

import numpy as np
import pytest

import issref
import matchref as mr
import mvicp
import offorigin as oo
import traverseref
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
WIDTH = {"idx": 1, "xyz": 3, "saliency": 1, "cnt_salient": 1, "cnt_nms": 1}


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def assert_same(got, want, what):
    for key, dt in issref.KEYS:
        a = got[key].cpu().numpy() if isinstance(got[key], torch.Tensor) else got[key]
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(want[key])
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape, (what, key, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            rows = np.unique(bad // WIDTH[key])
            raise AssertionError((what, key, len(bad), len(rows), rows[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), b.reshape(-1)[bad[:4]].tolist()))


# ---- the five cases of tests/test_iss_cpu.py
@pytest.mark.parametrize("name", issref.CASES)
def test_case(eng, name):
    p, args = issref.case(name)
    want = issref.reference(name)
    assert len(want["idx"]) > 0
    eng.set_frames([p], None)
    assert_same(eng.iss_keypoints(0, *args), want, name)


# ---- away from the origin
PLACED = {"local": ("local", None), "local1e6": ("local1e6", None), "utm": ("unit", oo.WU), "mm_local": ("mm_local", None), "mm_utm": ("mm_local", oo.WU)}


@pytest.mark.parametrize("name", sorted(PLACED))
def test_away_from_the_origin(eng, name):
    p, (rs, rn, g21, g32, mn) = issref.case("bump")
    placement, extra = PLACED[name]
    q = oo.place_points(placement, p, shift_extra=extra)
    s = oo.place_scale(placement)
    assert np.abs(q).max() > 400.0 and np.ptp(q, axis=0).max() < 1.5
    want = issref.iss(q, s * rs, s * rn, g21, g32, mn)
    assert len(want["idx"]) > 20 and (q - q[0]).tobytes() != (s * (p - p[0])).tobytes()   # the placement rounds the coordinates: another input
    eng.set_frames([q], None)
    assert_same(eng.iss_keypoints(0, s * rs, s * rn, g21, g32, mn), want, name)


# ---- a handful of points, all within one radius
@pytest.mark.parametrize("n", [0, 1, 5, 63])
def test_few_points(eng, n):
    p = np.random.Generator(np.random.PCG64(9)).uniform(0.0, 0.05, size=(n, 3))
    want = issref.iss(p, 0.1, 0.1, 0.975, 0.975, 1)
    assert (want["cnt_salient"] == n).all() and len(want["idx"]) == (1 if n > 1 else 0)
    eng.set_frames([p], None)
    assert_same(eng.iss_keypoints(0, 0.1, 0.1, 0.975, 0.975, 1), want, n)
    assert_same(eng.iss_keypoints(0, 0.1, 0.1, 0.975, 0.975, 1, device=True), want, (n, "device"))


# ---- the ways out of the traversal (tests/traverseref.py)
SEP = 1000.0


def far_cloud(n_cluster, n_alone, seed, corners=False):
    """two patches of the bump surface, 0.3 wide and SEP apart along the diagonal, and points on their own between and around them;
    corners: also the eight corners of a box around everything, so that neither patch lies at a face of the grid"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = mr.bumps(n_cluster, seed, 0.0, 0.3)[0] * np.array([1.0, 0.3, 1.0])
    b = mr.bumps(n_cluster, seed + 1, 0.0, 0.3)[0] * np.array([1.0, 0.3, 1.0]) + SEP / np.sqrt(3.0)
    alone = rng.uniform(-0.15 * SEP, 0.75 * SEP, size=(n_alone, 3))
    parts = [a, alone, b]
    if corners:
        parts.append(np.array([[x, y, z] for x in (-0.2, 0.8) for y in (-0.2, 0.8) for z in (-0.2, 0.8)]) * SEP)
    p = np.concatenate(parts, 0)
    return np.ascontiguousarray(p[rng.permutation(len(p))])


@pytest.mark.parametrize("kind", ["tree", "cloud"])
def test_far_clusters_take_the_other_ways_out(eng, kind):
    """The radius is chosen from the cell edge of the grid the library built: 5.2 cells leave the block of radius 4 unfinished (n >= 365:
    that block is below 2 n cells) and the lane goes to the box tree; 2.6 cells in a cloud of 132 points leave the block of radius 2
    unfinished (a face of that block is at most 2.5 cells away) and the block of radius 3 has 343 > 2 n cells, so the cloud itself is
    scanned -- unless the block is cut off by a face of the grid, which is why that cloud has points at the corners of a box around it.
    The two clusters are more than 1e3 radii apart in the first cloud; in the second the grid of so few points is too coarse for that
    (the cell edge follows the extent: the heuristic stops after three corrections), and they are more than 20 radii apart."""
    p = far_cloud(500, 6, 21) if kind == "tree" else far_cloud(60, 4, 23, corners=True)
    n = len(p)
    eng.set_frames([p], None)
    sc = eng.get_structure(0, "scalars")
    radius = (5.2 if kind == "tree" else 2.6) * float(sc[6])
    assert SEP > (1e3 if kind == "tree" else 20.0) * radius and eng.get_structure(0, "oct").size > 0
    ways = traverseref.exits(p, sc, n, radius)[0]
    print(kind, "cell", sc[6], "dims", sc[:3], {w: ways.count(w) for w in set(ways)})
    assert ways.count(kind) > 0.5 * n
    want = issref.iss(p, radius, 0.5 * radius, 0.975, 0.975, 3)
    assert len(want["idx"]) > 0 and (want["cnt_salient"] == 1).sum() >= 5 and want["cnt_salient"].max() > 20
    assert_same(eng.iss_keypoints(0, radius, 0.5 * radius, 0.975, 0.975, 3), want, kind)
    # the second pass at the large radius, the first at the small one
    want = issref.iss(p, 0.5 * radius, radius, 0.975, 0.975, 3)
    assert_same(eng.iss_keypoints(0, 0.5 * radius, radius, 0.975, 0.975, 3), want, (kind, "swapped"))


# ---- destinations
def test_host_and_device_destinations(eng):
    p, args = issref.case("bump")
    nrm = mr.e2e_clouds()["src_nrm"]
    want = issref.reference("bump")
    eng.set_frames([p], [nrm])
    host, dev = eng.iss_keypoints(0, *args), eng.iss_keypoints(0, *args, device=True)
    assert all(isinstance(dev[key], torch.Tensor) and dev[key].is_cuda for key, _ in issref.KEYS)
    assert_same(host, want, "host"); assert_same(dev, want, "device")
    k, n = len(want["idx"]), len(p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    xyz, nr = np.zeros((k, 3)), np.zeros((k, 3))
    assert eng.lib.mvicp_iss_fetch(eng.h, k, None, vp(xyz), vp(nr), 0, None, None, None) == 0
    assert xyz.tobytes() == np.ascontiguousarray(p[want["idx"]]).tobytes() and nr.tobytes() == np.ascontiguousarray(nrm[want["idx"]]).tobytes()
    d_nr = torch.zeros((k, 3), dtype=torch.float64, device=dev["idx"].device)
    cn = np.zeros(n, np.int32)
    torch.cuda.synchronize()
    assert eng.lib.mvicp_iss_fetch(eng.h, k, None, None, C.c_void_p(d_nr.data_ptr()), n, None, None, vp(cn)) == 0   # one device, one host pointer
    assert d_nr.cpu().numpy().tobytes() == nr.tobytes() and cn.tobytes() == want["cnt_nms"].tobytes()


# ---- the other results stay
def test_other_results_are_untouched(eng):
    p, args = issref.case("bump")
    nrm = mr.e2e_clouds()["src_nrm"]
    eng.set_frames([p], [nrm])
    n = len(p)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def fetch_both():
        desc, used = np.zeros((n, 33)), np.zeros(n, np.int32)
        assert eng.lib.mvicp_fpfh_fetch(eng.h, n, vp(desc), vp(used)) == 0
        cnt, off, idx, d2 = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros((n, 16), np.int32), np.zeros((n, 16))
        assert eng.lib.mvicp_knn_fetch(eng.h, n, n * 16, vp(cnt), vp(off), vp(idx), vp(d2)) == 0
        return desc.tobytes(), used.tobytes(), cnt.tobytes(), off.tobytes(), idx.tobytes(), d2.tobytes()

    eng.fpfh(0, args[0], 16)
    before = fetch_both()
    assert_same(eng.iss_keypoints(0, *args), issref.reference("bump"), "between")
    assert fetch_both() == before
    # and the keypoints survive a search and descriptors
    eng.knn_search(0, None, 8, 0.5 * args[0]); eng.fpfh(0, 0.7 * args[0], 32)
    k = len(issref.reference("bump")["idx"])
    idx = np.zeros(k, np.int32)
    assert eng.lib.mvicp_iss_fetch(eng.h, k, vp(idx), None, None, 0, None, None, None) == 0 and idx.tobytes() == issref.reference("bump")["idx"].tobytes()


def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_iss):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_iss:
                e.iss_keypoints(2, 0.05, 0.02)   # before the graph exists
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_iss:
                    e.iss_keypoints(r, 0.04, 0.02, 0.9, 0.9, 3)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_iss:
                    e.iss_keypoints(3 - r, (0.03, 0.06, 0.02)[r], (0.01, 0.03, 0.02)[r], device=(r == 2))
                triples, offsets = e.map_correspondences()
                epochs = e.correspondence_epochs()
                blocks = e.linearize(poses, True, True)
                poses, sm = e.optimize(poses, pb["fixed"])
                if with_iss:
                    e.iss_keypoints(r + 1, 0.05, 0.015)   # between rounds
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            epochs.tobytes(), sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


# ---- errors
def test_errors_and_empty_frames():
    p, args = issref.case("bump")
    args = (2.0 * args[0], 2.0 * args[1]) + args[2:]   # (300 of the 1500 points: twice the radii give 13 keypoints)
    small = np.ascontiguousarray(p[:300])
    nrm = np.ascontiguousarray(mr.e2e_clouds()["src_nrm"][:300])
    crowd = np.random.Generator(np.random.PCG64(9)).uniform(0.0, 0.01, size=(1100, 3))
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        idx, sal = np.zeros(300, np.int32), np.zeros(300)
        fetch_idx = lambda cap: lib.mvicp_iss_fetch(h, cap, vp(idx), None, None, 0, None, None, None)
        assert fetch_idx(300) == ERR_STATE and b"mvicp_iss_keypoints first" in lib.mvicp_last_error()   # before any call
        assert lib.mvicp_iss_keypoints(h, 0, *args) == ERR_ARG                                            # frames not declared: out of range
        assert lib.mvicp_set_num_frames(h, 5) == 0
        assert lib.mvicp_set_frame(h, 0, dp(small), None, 300) == 0                                       # no normals
        assert lib.mvicp_set_frame(h, 1, dp(small), dp(nrm), 300) == 0
        empty = np.zeros((0, 3))
        assert lib.mvicp_set_frame(h, 2, dp(empty), dp(empty), 0) == 0
        assert lib.mvicp_set_frame(h, 4, dp(crowd), None, 1100) == 0
        assert lib.mvicp_iss_keypoints(h, 3, *args) == ERR_STATE and b"never uploaded" in lib.mvicp_last_error()
        assert fetch_idx(300) == ERR_STATE
        want = issref.iss(small, *args)
        k = len(want["idx"])
        assert 3 < k < 300 and lib.mvicp_iss_keypoints(h, 0, *args) == k
        assert fetch_idx(k - 1) == ERR_ARG and b"cap_keys" in lib.mvicp_last_error()
        assert lib.mvicp_iss_fetch(h, 0, None, None, None, 299, vp(sal), None, None) == ERR_ARG and b"cap_n" in lib.mvicp_last_error()
        xyz = np.zeros((300, 3))
        assert lib.mvicp_iss_fetch(h, 300, None, None, vp(xyz), 0, None, None, None) == ERR_STATE and b"normals" in lib.mvicp_last_error()
        assert fetch_idx(k) == 0 and idx[:k].tobytes() == want["idx"].tobytes()
        assert lib.mvicp_iss_fetch(h, 0, None, None, None, 300, vp(sal), None, None) == 0 and sal.tobytes() == want["saliency"].tobytes()
        # an argument error leaves the last result alone
        for bad in ((0, 0.0, 0.1, 0.9, 0.9, 5), (0, 0.1, float("nan"), 0.9, 0.9, 5), (0, 0.1, 0.1, 0.0, 0.9, 5), (0, 0.1, 0.1, 0.9, float("inf"), 5),
                    (0, 0.1, 0.1, 0.9, 0.9, 0), (0, 0.1, 0.1, 0.9, 0.9, 1025), (0, 2.0 ** -301, 0.1, 0.9, 0.9, 5), (0, 0.1, 2.0 ** 301, 0.9, 0.9, 5), (7, 0.1, 0.1, 0.9, 0.9, 5)):
            assert lib.mvicp_iss_keypoints(h, *bad) == ERR_ARG, bad
        idx[:] = 0
        assert fetch_idx(k) == 0 and idx[:k].tobytes() == want["idx"].tobytes()
        assert lib.mvicp_iss_keypoints(h, 1, *args) == k
        assert lib.mvicp_iss_fetch(h, 300, None, None, vp(xyz), 0, None, None, None) == 0 and xyz[:k].tobytes() == np.ascontiguousarray(nrm[want["idx"]]).tobytes()
        # more than 1024 points within the salient radius: reported by the call, and no result is left behind
        assert lib.mvicp_iss_keypoints(h, 4, 0.1, 0.1, 0.975, 0.975, 5) == ERR_ARG and b"1024" in lib.mvicp_last_error()
        assert fetch_idx(300) == ERR_STATE
        assert lib.mvicp_iss_keypoints(h, 4, 0.001, 0.1, 0.975, 0.975, 5) >= 0   # (only the salient radius is capped)
        # n = 0: no keypoint, no error
        assert lib.mvicp_iss_keypoints(h, 2, *args) == 0
        assert lib.mvicp_iss_fetch(h, 0, None, None, None, 0, None, None, None) == 0
        assert lib.mvicp_iss_keypoints(h, 1, *args) == k
        assert lib.mvicp_set_num_frames(h, 1) == 0                                                        # the result ends with the frames
        assert lib.mvicp_iss_fetch(h, 1 << 20, None, None, None, 1 << 20, None, None, None) == ERR_STATE
        # the same through the Engine, which keeps the sizes of the frames it uploaded
        fresh.set_frames([small, empty], None)
        got = fresh.iss_keypoints(1, *args)
        assert got["idx"].shape == (0,) and got["xyz"].shape == (0, 3) and got["saliency"].shape == (0,)
        got = fresh.iss_keypoints(1, *args, device=True)
        assert tuple(got["idx"].shape) == (0,) and tuple(got["xyz"].shape) == (0, 3)
        assert_same(fresh.iss_keypoints(0, *args), want, "300 points")
    finally:
        fresh.close()
