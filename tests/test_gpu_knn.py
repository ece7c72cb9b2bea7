"""mvicp_knn_search / mvicp_knn_fetch on the MI355X: cnt, off, idx, d2 and the returned total equal the numpy statement of the contract
(tests/knnref.py) byte for byte; no tolerance anywhere.  What a case must contain (ties cut by k, saturated / partly filled / empty rows,
rows longer than any list) is asserted on the reference alone, so no case can pass trivially."""
import ctypes as C
import functools

import numpy as np
import pytest

import knnref
import mvicp
import offorigin as oo
import outlierref
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
    assert int(got["total"]) == int(want["total"]), (what, "total", got["total"], want["total"])
    for key, dt in knnref.KEYS:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape, (what, key, a.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1))
            rows = np.unique(bad // (a.shape[1] if a.ndim == 2 else 1))
            raise AssertionError((what, key, len(bad), rows[:4].tolist(), a.reshape(-1)[bad[:4]].tolist(), b.reshape(-1)[bad[:4]].tolist()))


# ---- case 1: a uniform cloud and queries of every kind
@functools.lru_cache(maxsize=None)
def cloud1():
    return np.random.Generator(np.random.PCG64(1)).uniform(0.0, 1.0, size=(3000, 3))


_case1 = {}


def case1(eng):
    """-> (cloud, the 2000 queries, sorted rows of the reference); the engine holds the cloud as frame 0 afterwards."""
    p = cloud1()
    eng.set_frames([p], None)
    if "q" not in _case1:
        sc = eng.get_structure(0, "scalars")
        dims, origin, cell = sc[:3].astype(np.int64), sc[3:6], float(sc[6])
        rng = np.random.Generator(np.random.PCG64(11))
        uni = rng.uniform(-0.1, 1.1, size=(1500, 3))
        copies = p[rng.choice(len(p), size=200, replace=False)]
        faces = rng.uniform(0.0, 1.0, size=(200, 3))
        on = rng.integers(1, 8, size=200)   # which axes sit on a face plane: a non-empty subset
        for a in range(3):
            plane = origin[a] + rng.integers(0, dims[a] + 1, size=200) * cell
            faces[:, a] = np.where((on >> a) & 1, plane, faces[:, a])
        dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [-1, 1, -1], [1, -1, -1], [-1, -1, 1]], dtype=np.float64)
        far = 0.5 + dirs[np.arange(100) % len(dirs)] * rng.uniform(1.0, 50.0, size=(100, 1))
        far[:len(dirs)] = 0.5 + dirs * 50.0
        _case1["q"] = np.ascontiguousarray(np.vstack([uni, copies, faces, far]))
        _case1["faces_on_planes"] = int((on > 0).sum())
        _case1["sorted"] = knnref.sorted_rows(p, _case1["q"])
    return p, _case1["q"], _case1["sorted"]


@functools.lru_cache(maxsize=None)
def _ref1(k, radius):
    return knnref.from_sorted(*_case1["sorted"], k, radius)


@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 32, 33, 64])
def test_capacity_sweep(eng, k):
    """k = 8 | 9, 16 | 17, 32 | 33 straddle the list capacities; 2000 queries are 16 workgroups of 128 lanes (32 of 64 at capacity 64)."""
    p, q, _ = case1(eng)
    assert len(q) == 2000 and _case1["faces_on_planes"] == 200
    want = _ref1(k, 0.0)
    assert (want["cnt"] == k).all() and (want["d2"][1500:1700, 0] == 0).all()          # the copies find their point at +0
    assert want["d2"][1900:, 0].min() > 0.25 and want["d2"][1900:1910, 0].min() > 49.0 ** 2   # the far ones are far
    assert_same(eng.knn_search(0, q, k), want, ("sweep", k))


# ---- ties
@functools.lru_cache(maxsize=None)
def lattice_case():
    p = knnref.shuffled_lattice(7, 3)
    inner = p[((p >= 1) & (p <= 5)).all(1)]     # 125 points whose cell / face centres have every neighbour of the next two shells in the lattice
    corners = np.array([[x, y, z] for x in (0.0, 6.0) for y in (0.0, 6.0) for z in (0.0, 6.0)])
    q = np.ascontiguousarray(np.vstack([p[::3], inner[:50] + 0.5, inner[50:100] + [0.5, 0.5, 0.0], inner[100:125] + [0.0, 0.5, 0.5], corners,
                                        inner[:40] + [0.5, 0.0, 0.0]]))
    kinds = np.concatenate([np.zeros(len(p[::3])), np.ones(50), np.full(75, 2), np.full(8, 3), np.full(40, 4)]).astype(int)
    # kinds: 0 lattice point, 1 cell centre, 2 face centre, 3 lattice corner, 4 edge centre
    return p, q, kinds, knnref.sorted_rows(p, q)


def test_ties_are_cut_by_lowest_index(eng):
    p, q, kinds, srt = lattice_case()
    assert len(p) == 343 and not (np.lexsort(p.T[::-1]) == np.arange(343)).all()   # index order is unrelated to space
    want = knnref.from_sorted(*srt, 4, 0.0)
    order, Ds = srt
    centre, face, edge = kinds == 1, kinds == 2, kinds == 4
    interior = (kinds == 0) & ((q >= 1).all(1) & (q <= 5).all(1))
    assert (Ds[centre, :8] == 0.75).all() and (Ds[centre, 8] > 0.75).all()                        # 8 corners at exactly 0.75: k = 4 cuts them
    assert (Ds[face, :4] == 0.5).all() and (Ds[face, 4:12] == 1.5).all() and (Ds[face, 12] > 1.5).all()   # 4, then 8: k = 6 cuts the 8
    assert (Ds[edge, :2] == 0.25).all() and (Ds[edge, 2:10] == 1.25).all() and (Ds[edge, 10] > 1.25).all()   # 2, then 8: k = 4 cuts the 8
    assert interior.sum() > 10 and (Ds[interior, 0] == 0).all() and (Ds[interior, 1:7] == 1).all()   # itself, then 6: k = 4 cuts the 6
    cut = Ds[:, 3] == Ds[:, 4]       # the 4th and the 5th value are equal: the cut tie group has more than one member
    assert cut[centre].all() and cut[edge].all() and cut[interior].all() and not cut[face].any()
    assert (want["d2"][centre] == 0.75).all() and (np.diff(want["idx"][centre], axis=1) > 0).all()    # the lowest indices, ascending
    for i in np.flatnonzero(centre)[:5]:
        assert want["idx"][i].tolist() == sorted(order[i, :8].tolist())[:4]
    eng.set_frames([p], None)
    assert_same(eng.knn_search(0, q, 4), want, "lattice k=4")
    want6 = knnref.from_sorted(*srt, 6, 0.0)    # face centres: 4 at 0.5, then 2 of the 8 at 1.5
    assert (want6["d2"][face, 4:] == 1.5).all() and (np.diff(want6["idx"][face, 4:], axis=1) > 0).all()
    assert_same(eng.knn_search(0, q, 6), want6, "lattice k=6")
    lat, _ = outlierref.lattice_cloud()
    assert outlierref.tie_count(lat, 8) == 108
    eng.set_frames([lat], None)
    assert_same(eng.knn_search(0, None, 8), knnref.knn_search(lat, None, 8), "12 x 12 x 2 lattice, self, k=8")


def test_strict_radius(eng):
    p, q, kinds, srt = lattice_case()
    eng.set_frames([p], None)
    interior = np.flatnonzero((kinds == 0) & ((q >= 1).all(1) & (q <= 5).all(1)))
    corner, centre = np.flatnonzero(kinds == 3), np.flatnonzero(kinds == 1)
    assert len(interior) > 10 and len(corner) == 8 and len(centre) == 50
    for radius, n_int, n_cor in ((1.0, 1, 1), (float(np.nextafter(1.0, 2.0)), 7, 4)):
        want = knnref.from_sorted(*srt, 0, radius)
        assert (want["cnt"][interior] == n_int).all() and (want["cnt"][corner] == n_cor).all() and (want["cnt"][centre] == 8).all()
        assert_same(eng.knn_search(0, q, 0, radius), want, ("strict", radius))


@pytest.mark.parametrize("k,radius", [(8, 0.08), (16, 0.10), (32, 0.13), (64, 0.16)])
def test_bounded_k_mode(eng, k, radius):
    p, q, _ = case1(eng)
    want = _ref1(k, radius)
    cnt = want["cnt"]
    assert (cnt == k).sum() > 0 and ((cnt > 0) & (cnt < k)).sum() > 0 and (cnt == 0).sum() > 0    # saturated, partly filled, empty
    pad = np.arange(k)[None, :] >= cnt[:, None]
    assert (want["idx"][pad] == -1).all() and np.isposinf(want["d2"][pad]).all() and not np.isinf(want["d2"][~pad]).any()
    got = eng.knn_search(0, q, k, radius)
    assert (got["idx"][pad] == -1).all() and (got["d2"][pad].view(np.uint64) == np.float64(np.inf).view(np.uint64)).all()   # the padding bytes
    assert_same(got, want, ("bounded", k, radius))


def test_all_mode(eng):
    p, q, _ = case1(eng)
    want = _ref1(0, 0.25)
    assert (want["cnt"] > 64).sum() > 1000 and want["cnt"].max() > 200 and (want["cnt"] == 0).sum() > 0 and want["total"] > 150000
    got = eng.knn_search(0, q, 0, 0.25)
    assert got["idx"].shape == (want["total"],) and got["off"][-1] == want["total"]
    assert_same(got, want, "all, 0.25")
    assert_same(eng.knn_search(0, None, 0, 0.05), knnref.knn_search(p, None, 0, 0.05), "all, self, 0.05")


def test_degenerate_sizes(eng):
    same_pts = np.tile([[0.25, -0.5, 1.0]], (20, 1))
    five = np.random.Generator(np.random.PCG64(4)).uniform(-1, 1, size=(5, 3))
    probe = np.array([[0.25, -0.5, 1.0], [3.0, 0.0, -2.0], [0.0, 0.0, 0.0]])
    eng.set_frames([same_pts, five, five[:1], np.zeros((0, 3))], None)
    got = eng.knn_search(0, None, 8)
    assert (got["idx"] == np.arange(8)).all() and (got["d2"] == 0).all() and not np.signbit(got["d2"]).any() and (got["cnt"] == 8).all()
    assert_same(got, knnref.knn_search(same_pts, None, 8), "identical, self")
    assert_same(eng.knn_search(0, probe, 8, 0.5), knnref.knn_search(same_pts, probe, 8, 0.5), "identical, probes")
    got = eng.knn_search(1, probe, 8)
    assert (got["cnt"] == 5).all() and (got["idx"][:, 5:] == -1).all() and np.isposinf(got["d2"][:, 5:]).all()
    assert_same(got, knnref.knn_search(five, probe, 8), "n = 5 < k")
    assert_same(eng.knn_search(1, None, 64), knnref.knn_search(five, None, 64), "n = 5, self, k = 64")
    assert_same(eng.knn_search(1, probe, 0, 2.0), knnref.knn_search(five, probe, 0, 2.0), "n = 5, all")
    for k, radius in ((1, 0.0), (8, 0.0), (0, 10.0), (0, 0.5)):
        assert_same(eng.knn_search(2, probe, k, radius), knnref.knn_search(five[:1], probe, k, radius), ("n = 1", k, radius))
        assert_same(eng.knn_search(2, None, k, radius), knnref.knn_search(five[:1], None, k, radius), ("n = 1, self", k, radius))
        got = eng.knn_search(3, probe, k, radius)                                    # an empty frame: no error, every row empty
        assert (got["cnt"] == 0).all() and got["total"] == 0
        assert_same(got, knnref.knn_search(np.zeros((0, 3)), probe, k, radius), ("n = 0", k, radius))
        assert_same(eng.knn_search(3, None, k, radius), knnref.knn_search(np.zeros((0, 3)), None, k, radius), ("n = 0, self", k, radius))
        got = eng.knn_search(1, np.zeros((0, 3)), k, radius)                         # no queries: an empty result
        assert got["cnt"].shape == (0,) and got["off"].tolist() == [0] and got["total"] == 0
        assert_same(got, knnref.knn_search(five, np.zeros((0, 3)), k, radius), ("m = 0", k, radius))


def test_self_mode_and_the_outlier_filter(eng):
    p = cloud1()
    p = np.ascontiguousarray(np.vstack([p, p[:50]]))     # 50 duplicated points: two candidates at distance 0
    eng.set_frames([p], None)
    srt = knnref.sorted_rows(p)
    for k in (8, 32):
        want = knnref.from_sorted(*srt, k + 1, 0.0)
        got = eng.knn_search(0, None, k + 1)
        assert_same(got, want, ("self", k + 1))
        assert_same(eng.knn_search(0, p, k + 1), want, ("the cloud as queries", k + 1))
        assert (got["d2"][:, 0] == 0).all() and (got["idx"][:50, 0] == np.arange(50)).all() and (got["idx"][3000:, 0] == np.arange(50)).all()
        kd2 = eng.outlier_filter(0, k, -1.0, 0.0)["kd2"]
        assert got["d2"][:, k].tobytes() == kd2.tobytes(), k


def test_against_nn_query(eng):
    p, q, (order, Ds) = case1(eng)
    got = eng.knn_search(0, q, 1)
    idx, d2 = eng.nn_query(0, q)
    assert got["d2"][:, 0].tobytes() == d2.tobytes()
    unique = Ds[:, 0] < Ds[:, 1]
    assert unique.sum() > 1900
    assert (got["idx"][unique, 0] == idx[unique]).all() and (idx[unique] == order[unique, 0]).all()


def test_structures_and_order_give_the_same_bytes(eng):
    p, q, _ = case1(eng)
    want = {(k, r): _ref1(k, r) for k, r in ((16, 0.0), (33, 0.13), (0, 0.15))}
    e = mvicp.Engine(0)
    try:
        for target in (1.0, 50.0):    # nearly empty cells: the block grows / crowded cells: long runs
            e.set_option("grid_target", target)
            for upload in ("host", "device"):
                if upload == "host":
                    e.set_frames([p], None)
                else:
                    e.set_frames_device([_dev(p)], None)
                for order_on in (1, 0):
                    e.set_option("knn_order", order_on)
                    for (k, r), w in want.items():
                        assert_same(e.knn_search(0, q, k, r), w, (target, upload, order_on, k, r))
                e.set_option("knn_order", 1)
    finally:
        e.close()


def test_device_in_device_out_and_errors(eng):
    p, q, _ = case1(eng)
    dq = _dev(q)
    for k, r in ((8, 0.0), (32, 0.13), (0, 0.15)):
        dev = eng.knn_search(0, dq, k, r, device=True)
        assert all(isinstance(dev[key], torch.Tensor) and dev[key].is_cuda for key in ("cnt", "off", "idx", "d2"))
        assert_same(dev, _ref1(k, r), ("device", k, r))
    assert_same(eng.knn_search(0, dq, 8, 0.0), _ref1(8, 0.0), "device in, host out")     # a second search refills
    lib, h = eng.lib, eng.h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    m = len(q)
    cnt, off, idx, d2 = np.zeros(m, np.int32), np.zeros(m + 1, np.int64), np.zeros(m * 8, np.int32), np.zeros(m * 8)
    assert lib.mvicp_knn_fetch(h, m - 1, m * 8, vp(cnt), None, None, None) == ERR_ARG and b"cap_rows" in lib.mvicp_last_error()
    assert lib.mvicp_knn_fetch(h, m - 1, m * 8, None, vp(off), None, None) == ERR_ARG
    assert lib.mvicp_knn_fetch(h, m, m * 8 - 1, None, None, vp(idx), None) == ERR_ARG and b"cap_entries" in lib.mvicp_last_error()
    assert lib.mvicp_knn_fetch(h, m, m * 8 - 1, None, None, None, vp(d2)) == ERR_ARG
    assert lib.mvicp_knn_fetch(h, 0, m * 8, None, None, vp(idx), vp(d2)) == 0            # (cap_rows is looked at only with cnt / off)
    assert lib.mvicp_knn_fetch(h, m, 0, vp(cnt), vp(off), None, None) == 0
    assert idx.reshape(m, 8).tobytes() == _ref1(8, 0.0)["idx"].tobytes() and off.tobytes() == _ref1(8, 0.0)["off"].tobytes()
    # an argument error leaves the last result alone
    assert lib.mvicp_knn_search(h, 0, vp(q), m, 65, 0.0) == ERR_ARG and lib.mvicp_knn_search(h, 0, vp(q), m, 0, 0.0) == ERR_ARG
    assert lib.mvicp_knn_search(h, 7, vp(q), m, 8, 0.0) == ERR_ARG
    assert lib.mvicp_knn_fetch(h, m, m * 8, vp(cnt), None, None, None) == 0 and (cnt == 8).all()
    # a non-finite query is reported by the search itself and leaves no result behind
    for bad in (np.nan, np.inf):
        for k, r in ((8, 0.0), (0, 0.1)):
            assert lib.mvicp_knn_search(h, 0, vp(q), m, 8, 0.0) == 8 * m
            qb = q.copy(); qb[1234, 1] = bad
            assert lib.mvicp_knn_search(h, 0, vp(qb), m, k, r) == ERR_ARG and b"not finite" in lib.mvicp_last_error()
            assert lib.mvicp_knn_fetch(h, m, m * 8, vp(cnt), None, None, None) == ERR_STATE
    fresh = mvicp.Engine(0)
    try:
        assert fresh.lib.mvicp_knn_fetch(fresh.h, 10, 10, None, None, None, None) == ERR_STATE      # a fetch before any search
        assert fresh.lib.mvicp_knn_search(fresh.h, 0, None, 0, 8, 0.0) == ERR_ARG                    # frames not declared: out of range
        assert fresh.lib.mvicp_set_num_frames(fresh.h, 2) == 0
        pp = np.ascontiguousarray(p[:300])
        assert fresh.lib.mvicp_set_frame(fresh.h, 0, pp.ctypes.data_as(C.POINTER(C.c_double)), None, len(pp)) == 0
        assert fresh.lib.mvicp_knn_search(fresh.h, 1, None, 0, 8, 0.0) == ERR_STATE and b"never uploaded" in fresh.lib.mvicp_last_error()
        assert fresh.lib.mvicp_knn_search(fresh.h, 0, None, 0, 8, 0.0) == 8 * 300
        assert fresh.lib.mvicp_set_num_frames(fresh.h, 1) == 0                                       # the result ends with the frames
        assert fresh.lib.mvicp_knn_fetch(fresh.h, 1 << 20, 1 << 30, None, None, None, None) == ERR_STATE
    finally:
        fresh.close()


def test_away_from_the_origin(eng):
    """UTM-sized coordinates in millimetre units: the cloud's extent is a millionth of its coordinates, and distances tie by rounding."""
    rng = np.random.Generator(np.random.PCG64(21))
    p = oo.place_points("mm_local", cloud1()[:2000], shift_extra=oo.WU)
    q = oo.place_points("mm_local", np.vstack([rng.uniform(-0.1, 1.1, size=(600, 3)), cloud1()[:100], [[30.0, 0.5, 0.5], [-20.0, -20.0, 20.0]]]), shift_extra=oo.WU)
    assert np.abs(p).max() > 4e6 and np.ptp(p, axis=0).max() < 2e-3
    srt = knnref.sorted_rows(p, q)
    for k, radius in ((16, 0.13e-3), (16, 0.0), (0, 0.13e-3)):
        want = knnref.from_sorted(*srt, k, radius)
        if radius > 0:
            c = want["cnt"]
            assert (c == 0).sum() > 0 and (c > 0).sum() > 300 and (k == 0 or ((c == k).sum() > 0 and ((c > 0) & (c < k)).sum() > 0))
        eng.set_frames([p], None)
        assert_same(eng.knn_search(0, q, k, radius), want, ("utm mm", k, radius))


def test_history_neutral():
    pb = synth.make_problem(4, 3000)
    probe = np.ascontiguousarray(pb["pts"][1][::7] + 0.003)

    def run(with_search):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_search:
                e.knn_search(2, None, 8)   # before the graph exists
                e.knn_search(0, probe, 0, 0.03)
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_search:
                    e.knn_search(r, probe, 16, 0.05)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_search:
                    e.knn_search(3 - r, None if r == 1 else probe, (33, 0, 1)[r], (0.0, 0.02, 0.0)[r], device=(r == 2))
                triples, offsets = e.map_correspondences()
                blocks = e.linearize(poses, True, True)
                poses, sm = e.optimize(poses, pb["fixed"])
                if with_search:
                    e.knn_search(r + 1, _dev(probe), 64)   # between rounds
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)
