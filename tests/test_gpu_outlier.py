"""mvicp_outlier_filter / mvicp_outlier_fetch on the MI355X: every array (xyz, nrm, idx, mdist, kd2) and every number of the stats equals
the numpy statement of the contract (tests/outlierref.py) byte for byte.  What a case must contain (outliers removed, ties, a block that
grows across the grid) is asserted on the reference alone, so no case can pass by keeping or dropping everything."""
import ctypes as C
import functools

import numpy as np
import pytest

import mvicp
import outlierref
import pathcases
import traverseref
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
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def assert_same(got, want, what):
    got = _host(got)
    assert (got["nrm"] is None) == (want["nrm"] is None), what
    for k, dt in (("idx", np.int32), ("mdist", np.float64), ("kd2", np.float64), ("xyz", np.float64), ("nrm", np.float64)):
        if want[k] is None:
            continue
        assert got[k].dtype == dt and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k]).astype(dt)
        bad = np.argwhere(a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1))[:, 0] if a.size else []
        assert a.tobytes() == b.tobytes(), (what, k, len(set(np.asarray(bad).tolist())), np.unique(bad)[:4].tolist())
    gs, ws = got["stats"], want["stats"]
    for k in ("n", "kept", "q_exp", "s1", "s2_hi", "s2_lo", "has_normals"):
        assert int(gs[k]) == int(ws[k]), (what, k, gs[k], ws[k])
    for k in ("T", "threshold"):
        assert np.float64(gs[k]).tobytes() == np.float64(ws[k]).tobytes(), (what, k, gs[k], ws[k])


@functools.lru_cache(maxsize=None)
def sheet(n):
    return outlierref.sheet_cloud(n, 100 + n)


@functools.lru_cache(maxsize=None)
def sheet_ref(n, k, std_ratio, radius, normals=True):
    p, nr, planted = sheet(n)
    return outlierref.outlier_filter(p, nr if normals else None, k, std_ratio, radius)


@pytest.mark.parametrize("k", pathcases.OUTLIER_SWEEP_K)
@pytest.mark.parametrize("n", ["k+1", 63, 64, 65, 257, 5000])
def test_size_sweep(eng, n, k):
    """n = k + 1 makes every list the whole cloud; 63 / 64 / 65 straddle a wave, 257 two workgroups of the knn kernel.  The knn kernel has
    three list capacities: k <= 8 runs <9>, 9 <= k <= 16 runs <17>, k >= 17 runs <33>; k = 1, 8 | 9, 16 | 17, 32 are the ends of the three
    ranges, so both sides of each boundary run (tests/test_paths_cpu.py holds the list against the dispatch in csrc/outlier.hip)."""
    assert pathcases.OUTLIER_SWEEP_K == pathcases.outlier_boundary_ks()
    n = k + 1 if n == "k+1" else n
    p, nr, planted = sheet(n)
    want = sheet_ref(n, k, 2.0, 0.0)
    if n >= 2000:   # on the reference alone: the rule removes a few per cent, and the planted points are among them
        removed = set(range(n)) - set(want["idx"].tolist())
        assert 0.005 * n <= len(removed) <= 0.05 * n, len(removed)
        assert len(removed & set(planted.tolist())) >= 0.85 * len(planted)
    eng.set_frames([p], [nr])
    assert_same(eng.outlier_filter(0, k, 2.0, 0.0), want, (n, k))


@pytest.mark.parametrize("n,kept", [(255, 237), (256, 229), (257, 239)])
def test_one_workgroup_of_the_compaction(eng, n, kept):
    """255 / 256 / 257 rows: one workgroup of the row compaction with a lane to spare, exactly full, and one point in a second one."""
    p, nr, planted = sheet(n)
    want = sheet_ref(n, 8, 1.0, 0.0)
    assert len(want["idx"]) == kept
    eng.set_frames([p], [nr])
    assert_same(eng.outlier_filter(0, 8, 1.0, 0.0), want, (n, "host"))
    assert_same(eng.outlier_filter(0, 8, 1.0, 0.0, device=True), want, (n, "device"))


@pytest.mark.parametrize("k,std_ratio,radius", pathcases.O1_PARAMS)
def test_far_from_the_origin(eng, k, std_ratio, radius):
    """O1: a cloud of 1 mm extent at UTM coordinates (|p| > 4e6, the spacing of the doubles there is a nanometre), one case per list
    capacity, the statistical rule, both rules and the radius rule alone."""
    want = pathcases.check_outlier_far(k, std_ratio, radius)
    p, nr = pathcases.outlier_far_cloud()
    eng.set_frames([p], [nr])
    assert_same(eng.outlier_filter(0, k, std_ratio, radius), want, ("far", k, std_ratio, radius))
    assert_same(eng.outlier_filter(0, k, std_ratio, radius, device=True), want, ("far, device fetch", k, std_ratio, radius))


def test_lattice_ties_and_a_far_cluster(eng):
    p, nr = outlierref.lattice_cloud()
    k = 8
    assert len(p) == 293 and outlierref.tie_count(p, k) == 108        # exact ties at the k-th place
    assert (p[:, 0] > 2.9).sum() == 5 < k + 1                           # the far cluster cannot fill a list: its block grows across the grid
    eng.set_frames([p], [nr])
    sc = eng.get_structure(0, "scalars")
    dims = sc[:3]
    assert dims.max() >= 8, dims
    # the knn kernel stops at the k+1-th reference distance and walks no box tree: the far cluster cannot stop (tests/traverseref.py)
    ways = traverseref.exits(p, sc, len(p), np.sqrt(outlierref.k_distances(p, k)[1]), tree=False)[0]
    print("lattice", "cell", sc[6], "dims", dims, {w: ways.count(w) for w in set(ways)}, "the far five:", ways[288:])
    assert all(w in ("cloud", "grid") for w in ways[288:]) and ways[:288].count("stop") > 200
    for std_ratio, radius in ((2.0, 0.0), (-1.0, 0.0076), (1.0, 0.0076)):
        want = outlierref.outlier_filter(p, nr, k, std_ratio, radius)
        assert 0 < want["stats"]["kept"] < len(p) and not (want["idx"] >= 288).any()
        assert_same(eng.outlier_filter(0, k, std_ratio, radius), want, ("lattice", std_ratio, radius))
    # the same cluster nearer by: another grid, fewer cells between the two
    q = np.vstack([p[:288], p[288:] - [2.6, 0.0, 0.0]])
    eng.set_frames([q], None)
    dims = eng.get_structure(0, "scalars")[:3]
    assert dims.max() >= 8, dims
    assert_same(eng.outlier_filter(0, k, 2.0, 0.0), outlierref.outlier_filter(q, None, k, 2.0, 0.0), "near cluster")


def test_identical_points(eng):
    p = np.tile([[0.25, -0.5, 1.0]], (100, 1))
    eng.set_frames([p], None)
    for radius in (0.0, 0.01):
        want = outlierref.outlier_filter(p, None, 8, 2.0, radius)
        assert want["stats"]["kept"] == 100 and want["stats"]["q_exp"] == 0 and want["stats"]["s1"] == 0 and (want["kd2"] == 0).all()
        assert_same(eng.outlier_filter(0, 8, 2.0, radius), want, ("identical", radius))


def test_points_on_a_line(eng):
    """A cloud without extent along two axes: the hash grid is one occupied layer thick there (its dimension is 2, the smallest the
    build gives: the occupied layer and the closing one), so every block is clamped on both sides of it."""
    rng = np.random.Generator(np.random.PCG64(9))
    t = np.sort(rng.uniform(0.0, 2.0, size=400))
    p = np.outer(t, [1.0, 0.0, 0.0]) + [0.5, -0.25, 3.0]
    p = p[rng.permutation(len(p))]
    eng.set_frames([p], None)
    sc = eng.get_structure(0, "scalars")
    dims = sc[:3]
    assert sorted(dims.tolist())[:2] == [2.0, 2.0] and dims.max() > 8, dims
    for k in (4, 16):
        want = outlierref.outlier_filter(p, None, k, 1.0, 0.0)
        assert 0 < want["stats"]["kept"] < len(p)
        # a face of the block at or beyond the grid's boundary does not enter the stop rule: points stop whose k+1-th distance exceeds
        # the distance to such a face's plane, which the rule over all six faces would have sent on to a larger block
        d = np.sqrt(want["kd2"])
        ways, radii, left_out = traverseref.exits(p, sc, len(p), d, tree=False)
        sooner = int(((np.array(ways) == "stop") & (d > left_out + 0.01 * sc[6])).sum())
        print("line", "k", k, "cell", sc[6], "dims", dims, {w: ways.count(w) for w in set(ways)}, "stop with a boundary face nearer than the k+1-th distance:", sooner)
        assert ways.count("stop") > 0.9 * len(p) and (sooner >= 1 or k == 4)
        assert_same(eng.outlier_filter(0, k, 1.0, 0.0), want, ("line", k))


@pytest.mark.parametrize("std_ratio,radius", [(0.0, 0.0), (-1.0, 0.08), (2.0, 0.08), (0.5, 0.06), (-1.0, 0.0), (-1.0, -1.0)])
def test_rules(eng, std_ratio, radius):
    """std_ratio = 0, the radius rule alone, both rules, neither rule."""
    n, k = 2000, 8
    p, nr, planted = sheet(n)
    want = sheet_ref(n, k, std_ratio, radius)
    kept = want["stats"]["kept"]
    if std_ratio < 0 and radius <= 0:
        assert kept == n and want["stats"]["q_exp"] == 0 and want["stats"]["s2_lo"] == 0      # a k-distance query
    else:
        assert 0.3 * n < kept < n and len(set(planted.tolist()) - set(want["idx"].tolist())) >= 0.85 * len(planted)
    if std_ratio >= 0 and radius > 0:   # both rules: what passes the one and the other
        a, b = sheet_ref(n, k, std_ratio, 0.0)["idx"], sheet_ref(n, k, -1.0, radius)["idx"]
        assert want["idx"].tolist() == sorted(set(a.tolist()) & set(b.tolist()))
    eng.set_frames([p], [nr])
    assert_same(eng.outlier_filter(0, k, std_ratio, radius), want, (std_ratio, radius))


def test_frame_without_normals_and_second_frame(eng):
    n, k = 2000, 8
    p, nr, _ = sheet(n)
    p2, nr2, _ = sheet(257)
    eng.set_frames([p2, p], [nr2, None])
    got = eng.outlier_filter(1, k, 2.0, 0.0)
    assert got["nrm"] is None
    assert_same(got, sheet_ref(n, k, 2.0, 0.0, False), "no normals")
    buf = np.zeros((n, 3))
    st = eng.lib.mvicp_outlier_fetch(eng.h, n, None, buf.ctypes.data_as(C.c_void_p), None, 0, None, None)
    assert st == ERR_STATE and b"normals" in eng.lib.mvicp_last_error()
    assert_same(eng.outlier_filter(0, k, 2.0, 0.0), sheet_ref(257, k, 2.0, 0.0), "frame 0 of two")


def test_host_and_device_upload_agree_and_device_destinations_refill(eng):
    n, k = 5000, 8
    p, nr, _ = sheet(n)
    want = sheet_ref(n, k, 2.0, 0.0)
    eng.set_frames_device([_dev(p)], [_dev(nr)])
    got = eng.outlier_filter(0, k, 2.0, 0.0)
    assert_same(got, want, "device upload")
    dev = eng.outlier_filter(0, k, 2.0, 0.0, device=True)
    assert all(isinstance(dev[key], torch.Tensor) and dev[key].is_cuda for key in ("xyz", "nrm", "idx", "mdist", "kd2"))
    assert_same(dev, want, "device fetch")
    # the device result goes straight into another engine; its structures equal those of the numpy result uploaded from the host, and a
    # second pass over the cleaned cloud equals the reference's second pass
    a, b = mvicp.Engine(0), mvicp.Engine(0)
    try:
        a.set_frames_device([dev["xyz"]], [dev["nrm"]])
        b.set_frames([got["xyz"]], [got["nrm"]])
        for name in ("spts", "snor", "sidx"):
            assert a.get_structure(0, name).tobytes() == b.get_structure(0, name).tobytes(), name
        again = outlierref.outlier_filter(want["xyz"], want["nrm"], k, 2.0, 0.0)
        assert_same(a.outlier_filter(0, k, 2.0, 0.0), again, "second pass, device")
        assert_same(b.outlier_filter(0, k, 2.0, 0.0), again, "second pass, host")
    finally:
        a.close(); b.close()


def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_filter):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_filter:
                e.outlier_filter(2, 8, 2.0, 0.0)   # before the graph exists
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_filter:
                    e.outlier_filter(r, 16, 2.0, 0.0)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_filter:
                    e.outlier_filter(3 - r, 8 if r else 32, -1.0 if r == 1 else 1.0, 0.02, device=(r == 2))
                triples, offsets = e.map_correspondences()
                blocks = e.linearize(poses, True, True)
                poses, sm = e.optimize(poses, pb["fixed"])
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_errors_and_empty_frame(eng):
    p, nr, _ = sheet(257)
    fresh = mvicp.Engine(0)
    try:
        filt, fetch = fresh.lib.mvicp_outlier_filter, fresh.lib.mvicp_outlier_fetch
        assert fetch(fresh.h, 10, None, None, None, 10, None, None) == ERR_STATE      # a fetch before any filter call
        assert filt(fresh.h, 0, 8, 2.0, 0.0, None) == ERR_ARG                         # frames not declared: out of range
        assert fresh.lib.mvicp_set_num_frames(fresh.h, 3) == 0
        q = np.ascontiguousarray(p)
        assert fresh.lib.mvicp_set_frame(fresh.h, 0, q.ctypes.data_as(C.POINTER(C.c_double)), None, len(q)) == 0
        assert fresh.lib.mvicp_set_frame(fresh.h, 2, q.ctypes.data_as(C.POINTER(C.c_double)), None, 8) == 0
        assert filt(fresh.h, 1, 8, 2.0, 0.0, None) == ERR_STATE and b"never uploaded" in fresh.lib.mvicp_last_error()
        assert filt(fresh.h, 3, 8, 2.0, 0.0, None) == ERR_ARG and filt(fresh.h, -1, 8, 2.0, 0.0, None) == ERR_ARG
        assert filt(fresh.h, 2, 8, 2.0, 0.0, None) == ERR_ARG and b"more than k" in fresh.lib.mvicp_last_error()   # 0 < n <= k
        assert filt(fresh.h, 2, 7, -1.0, 0.0, None) == 8                               # n = k + 1 is fine
        assert fetch(fresh.h, 10, None, None, None, 10, None, None) == 0
        assert filt(fresh.h, 0, 0, 2.0, 0.0, None) == ERR_ARG and filt(fresh.h, 0, 33, 2.0, 0.0, None) == ERR_ARG
        assert fetch(fresh.h, 10, None, None, None, 10, None, None) == 0              # (an argument error leaves the last result alone)
        kept = filt(fresh.h, 0, 8, 2.0, 0.0, None)
        assert 1 < kept < len(q)
        buf, md = np.zeros((len(q), 3)), np.zeros(len(q))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert fetch(fresh.h, kept - 1, vp(buf), None, None, 0, None, None) == ERR_ARG        # cap_kept < kept
        assert fetch(fresh.h, kept, None, None, None, len(q) - 1, vp(md), None) == ERR_ARG    # cap_n < n
        assert fetch(fresh.h, kept, vp(buf), None, None, len(q), vp(md), None) == 0
        want = outlierref.outlier_filter(p, None, 8, 2.0, 0.0)
        assert buf[:kept].tobytes() == want["xyz"].tobytes() and md.tobytes() == want["mdist"].tobytes()
        assert fresh.lib.mvicp_set_num_frames(fresh.h, 1) == 0                                 # the result ends with the frames
        assert fetch(fresh.h, 1 << 20, None, None, None, 1 << 20, None, None) == ERR_STATE
    finally:
        fresh.close()
    eng.set_frames([np.zeros((0, 3)), p], None)
    got = eng.outlier_filter(0, 8, 2.0, 0.0)
    assert got["xyz"].shape == (0, 3) and got["idx"].shape == (0,) and got["mdist"].shape == (0,) and got["stats"]["kept"] == 0 and got["stats"]["n"] == 0
    got = eng.outlier_filter(0, 8, 2.0, 0.0, device=True)
    assert got["xyz"].shape == (0, 3) and got["kd2"].shape == (0,)
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        eng.outlier_filter(1, 8, float("nan"), 0.0)
