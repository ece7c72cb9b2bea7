"""mvicp_overlap on the MI355X: exact against the brute-force oracle (hits, sumq, q_exp as integers), independent of how the clouds were
built, history-neutral inside a registration, and the graph it yields where the pose rule fails."""
import ctypes as C
import math
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


def sqrt_bound(t):
    """smallest double x whose correctly rounded sqrt is >= t (the cutoff predicate sqrt(d2) < t as d2 < x)."""
    x = t * t
    while math.sqrt(x) >= t and x > 0.0:
        x = math.nextafter(x, 0.0)
    while math.sqrt(x) < t:
        x = math.nextafter(x, math.inf)
    return x


def q_exp_of(thresh):
    B2 = sqrt_bound(float(np.float32(thresh)))
    q = 31 - math.frexp(B2)[1]
    assert 2.0 ** 30 <= math.ldexp(B2, q) < 2.0 ** 31
    return q


def census_from_d2(d2_of_pair, npts, thresh, max_samples):
    """The definition, from per-pair arrays of nearest squared distances of ALL source points (d2_of_pair(i, j) -> n_i doubles)."""
    K = len(npts)
    t = float(np.float32(thresh))
    q = q_exp_of(thresh)
    samples = np.array([len(L.overlap_sample_indices(n, max_samples)) for n in npts], dtype=np.int32)
    hits = np.zeros((K, K), dtype=np.int32); sumq = np.zeros((K, K), dtype=np.int64)
    for i in range(K):
        hits[i, i] = samples[i]
        idx = L.overlap_sample_indices(npts[i], max_samples)
        for j in range(K):
            if i == j or npts[i] == 0 or npts[j] == 0:
                continue
            d2 = d2_of_pair(i, j)[idx]
            sel = np.sqrt(d2) < t                         # the predicate of frame.cpp:156
            hits[i, j] = int(sel.sum())
            sumq[i, j] = int(np.floor(np.ldexp(d2[sel], q)).astype(np.int64).sum())
    return samples, hits, sumq, q


class PairD2:
    """nn_d2 of the brute-force oracle for every ordered pair, computed once (orc.correspond_edge(...)[-1])."""

    def __init__(self, orc, pts, poses):
        self.orc, self.pts, self.poses, self.memo = orc, pts, poses, {}

    def __call__(self, i, j):
        if (i, j) not in self.memo:
            self.memo[(i, j)] = self.orc.correspond_edge(self.pts[i], self.poses[i], self.pts[j], self.poses[j], 0.05)[-1]
        return self.memo[(i, j)]


def assert_census_equal(got, want, what):
    samples, hits, sumq, q = want
    assert got["q_exp"] == q, what
    assert np.array_equal(got["samples"], samples), what
    assert np.array_equal(got["hits"], hits), (what, np.argwhere(got["hits"] != hits)[:5].tolist())
    assert np.array_equal(got["sumq"], sumq), (what, np.argwhere(got["sumq"] != sumq)[:5].tolist())
    K = len(samples)
    assert np.array_equal(got["fraction"], hits / np.maximum(samples, 1)[:, None])
    assert got["mean_d2"].shape == (K, K)


@pytest.fixture(scope="module")
def synth6(orc):
    pb = synth.make_problem(6, 20000, cone_deg=40)
    return pb, PairD2(orc, pb["pts"], pb["init"])


@pytest.fixture(scope="module")
def bunny4(orc):
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny18.npz"))
    off = g["row_off"]
    pts = [g["xyz_e8"][off[k]:off[k + 1]].astype(np.float64) / 1e8 for k in range(4)]
    poses = np.array(g["init"][:4], dtype=np.float64)
    return pts, poses, PairD2(orc, pts, poses)


# ---- 4. exact against the oracle
def test_exact_against_oracle_synthetic(synth6, orc, refnn):
    pb, d2 = synth6
    npts = [len(p) for p in pb["pts"]]
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        total = 0
        for thresh in (0.05, 0.01):
            for ms in (0, 1500):
                want = census_from_d2(d2, npts, thresh, ms)
                got = eng.overlap(pb["init"], thresh, ms)
                print("thresh", thresh, "max_samples", ms, "hits", got["hits"].tolist())
                assert_census_equal(got, want, (thresh, ms))
                total += int(want[1].sum() - want[0].sum())
        assert total > 0   # (the cases do have overlapping pairs)
        if refnn is not None:   # the same against the real nanoflann's d2 on the oracle's queries
            def ref_d2(i, j):
                return refnn.query(pb["pts"][j], orc.query_transform(pb["init"][i], pb["init"][j], pb["pts"][i]))[1]
            memo = {}
            want = census_from_d2(lambda i, j: memo.setdefault((i, j), ref_d2(i, j)), npts, 0.01, 1500)
            assert_census_equal(eng.overlap(pb["init"], 0.01, 1500), want, "nanoflann")
    finally:
        eng.close()


def test_exact_against_oracle_bunny_lattice_ties(bunny4):
    pts, poses, d2 = bunny4
    npts = [len(p) for p in pts]
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, None)
        for thresh in (0.05, 0.01):
            for ms in (0, 1500):
                got = eng.overlap(poses, thresh, ms)
                print("bunny thresh", thresh, "max_samples", ms, "hits", got["hits"].tolist())
                assert_census_equal(got, census_from_d2(d2, npts, thresh, ms), ("bunny", thresh, ms))
    finally:
        eng.close()


# ---- 5. the same answer however the clouds got there
def test_same_answer_for_every_build(synth6):
    pb, _ = synth6
    base = None
    for curve, target, device, async_build in [(2, 5.0, False, 1), (0, 5.0, False, 1), (1, 5.0, False, 0), (2, 3.0, False, 1), (2, 8.0, True, 1),
                                               (2, 5.0, True, 0), (1, 3.0, True, 1)]:
        eng = mvicp.Engine(0)
        try:
            eng.set_option("grid_curve", curve); eng.set_option("grid_target", target); eng.set_option("async_build", async_build)
            if device:
                eng.set_frames_device([_dev(p) for p in pb["pts"]], [_dev(n) for n in pb["nor"]])
            else:
                eng.set_frames(pb["pts"], pb["nor"])
            got = [eng.overlap(pb["init"], 0.01, ms) for ms in (0, 1500)]
        finally:
            eng.close()
        if base is None:
            base = got
            assert base[0]["hits"].sum() > base[0]["samples"].sum()
        for a, b in zip(base, got):
            for k in ("samples", "hits", "sumq", "q_exp"):
                assert np.array_equal(a[k], b[k]), (curve, target, device, async_build, k)


# ---- 6. history-neutral
def _register(pb, with_overlap, rounds=6):
    eng = mvicp.Engine(0)
    out = []
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        if with_overlap:
            eng.overlap(pb["init"], 0.05, 4096)   # before the graph exists
        eng.set_graph(pb["src"], pb["dst"])
        P = np.array(pb["init"])
        for rnd in range(rounds):
            if with_overlap:
                eng.overlap(P, 0.05, 4096 if rnd % 2 else 0)
            counts, weights = eng.correspond(P, pb["fixed"], 0.05)
            ep = eng.correspondence_epochs()
            if with_overlap:
                eng.overlap(P, 0.02, 1000)
            P, sm = eng.optimize(P, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
            out.append((counts.copy(), np.asarray(weights, np.float32).view(np.uint32).copy(), ep, P.copy(), sm))
    finally:
        eng.close()
    return out


def test_history_neutral():
    pb = synth.make_problem(8, 50000)
    plain, mixed = _register(pb, False), _register(pb, True)
    for rnd, (a, b) in enumerate(zip(plain, mixed)):
        assert np.array_equal(a[0], b[0]), rnd
        assert np.array_equal(a[1], b[1]), rnd
        assert np.array_equal(a[2], b[2]), rnd
        assert a[3].tobytes() == b[3].tobytes(), rnd
        assert a[4] == b[4], (rnd, a[4], b[4])


# ---- 7. the graph the pose rule misses
def test_finds_the_graph_the_pose_rule_misses(orc):
    K, N = 10, 20000
    pb = synth.make_problem(K, N, cone_deg=40)
    rng = np.random.Generator(np.random.PCG64(77))
    pts, poses = [pb["pts"][0]], [pb["gt"][0]]
    for k in range(1, K):
        D = np.eye(4)
        D[:3, :3] = synth.so3_exp(rng.normal(0, 1, 3))
        D[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        poses.append(pb["gt"][k] @ D)                              # pose_k = gt_k D_k
        pts.append((pb["pts"][k] - D[:3, 3]) @ D[:3, :3])          # p' = D_k^-1 p = R^T (p - t)
    poses = np.array(poses)
    thresh = np.float32(0.003)
    chain = {i: {j for j in (i - 1, i + 1) if 0 <= j < K} for i in range(K)}
    chain[0] = {1, 2}; chain[K - 1] = {K - 2, K - 3}
    ps, pd = synth.pose_graph_knn(poses, 2, skip_fixed0=False)
    pose_sets = {i: set(pd[ps == i].tolist()) for i in range(K)}
    assert pose_sets != chain   # the translation rule does not find it
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, None)
        for ms in (2048, 0):
            # the oracle's own hits first: a failure of the inputs must not pass for a failure of the kernel
            want = np.zeros((K, K), dtype=np.int64)
            samples = np.zeros(K, dtype=np.int64)
            for i in range(K):
                idx = L.overlap_sample_indices(N, ms)
                samples[i] = len(idx)
                for j in range(K):
                    if i != j:
                        d2 = orc.nn_brute(pts[j], orc.query_transform(poses[i], poses[j], pts[i][idx]))[1]
                        want[i, j] = int((np.sqrt(d2) < float(thresh)).sum())
            frac = want / samples[:, None]
            gaps = []
            for i in range(K):
                order = np.sort(frac[i])[::-1]
                gaps.append(order[1] - order[2])
                assert set(np.argsort(-frac[i], kind="stable")[:2].tolist()) == chain[i], (ms, i)
            print("max_samples", ms, "smallest gap between the 2nd and 3rd fraction", min(gaps))
            assert min(gaps) >= 0.1, (ms, gaps)
            got = eng.overlap(poses, thresh, ms)
            assert np.array_equal(got["hits"] - np.diag(np.diag(got["hits"])), want), ms
            src, dst, nc = mvicp.graph_from_overlap(got["samples"], got["hits"], got["sumq"], knn=2, skip_fixed0=False)
            sets = {i: set(dst[src == i].tolist()) for i in range(K)}
            assert sets == chain and nc == 1, (ms, sets, nc)
            assert sets != pose_sets
    finally:
        eng.close()


# ---- 8. edges of the definition
def _oracle_census(orc, pts, poses, thresh, ms):
    d2 = PairD2(orc, pts, poses)
    return census_from_d2(d2, [len(p) for p in pts], thresh, ms)


def test_far_apart_and_self_copy(orc):
    p = synth.make_view(0, 4, 20000)[0]
    eng = mvicp.Engine(0)
    try:
        I = np.eye(4)
        far = np.eye(4); far[0, 3] = 10.0
        eng.set_frames([p, p.copy()], None)
        got = eng.overlap([I, far], 0.05, 0)
        assert got["hits"].tolist() == [[20000, 0], [0, 20000]] and not got["sumq"].any()
        assert mvicp.graph_from_overlap(got["samples"], got["hits"], got["sumq"], knn=2, skip_fixed0=False)[2] == 2
        got = eng.overlap([I, I], 0.05, 0)                      # a cloud against its own copy at the same pose
        assert got["hits"].tolist() == [[20000, 20000], [20000, 20000]] and not got["sumq"].any()
        got = eng.overlap([I, I], 0.05, 50000)                  # max_samples larger than n
        assert got["samples"].tolist() == [20000, 20000] and got["hits"][0, 1] == 20000
    finally:
        eng.close()


def test_duplicates_empty_one_point_and_sub_leaf_clouds(orc):
    pb = synth.make_problem(2, 20000, cone_deg=40)
    big = pb["pts"][0]
    other = pb["pts"][1]
    dup = np.vstack([other[:3000], other[:3000], other[:100]])
    pts = [big, np.zeros((0, 3)), other[:1].copy(), other[100:170].copy(), dup]
    g, h = pb["gt"][0], pb["gt"][1]
    poses = np.array([g, h, h, h, h])
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, None)
        for thresh in (0.05, 0.004):
            for ms in (0, 64):
                got = eng.overlap(poses, thresh, ms)
                print("edge clouds thresh", thresh, "max_samples", ms, "hits", got["hits"].tolist())
                assert_census_equal(got, _oracle_census(orc, pts, poses, thresh, ms), (thresh, ms))
                assert got["samples"][1] == 0 and not got["hits"][1].any() and not got["hits"][:, 1].any()
        assert eng.overlap(poses, 0.05, 0)["hits"][3, 0] > 0
    finally:
        eng.close()


def test_scaled_and_shifted_clouds_match_the_oracle(orc):
    """Millimetre data far from the origin: the census reads only the sorted points and the outward-rounded box tree."""
    pb = synth.make_problem(3, 20000, cone_deg=40)
    shift = np.array([-50.0, -700.0, -470.0])
    pts = [p * 1000.0 + shift for p in pb["pts"]]
    poses = []
    for T in pb["init"]:
        S = T.copy()
        S[:3, 3] = 1000.0 * T[:3, 3] + shift - T[:3, :3] @ shift   # world' = 1000 world + shift for points p' = 1000 p + shift
        poses.append(S)
    poses = np.array(poses)
    thresh = np.float32(0.01) * np.float32(1000.0)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, None)
        for ms in (0, 1500):
            got = eng.overlap(poses, thresh, ms)
            want = _oracle_census(orc, pts, poses, thresh, ms)
            print("scaled max_samples", ms, "hits", got["hits"].tolist(), "oracle", want[1].tolist())
            assert want[1].sum() > want[0].sum()
            assert np.array_equal(got["hits"], want[1]), ms
    finally:
        eng.close()


# ---- 9. errors
def test_errors_and_the_context_still_works():
    pb = synth.make_problem(3, 3000)
    eng = mvicp.Engine(0)
    try:
        P = L.poses_to_c(pb["init"])
        samples = np.zeros(3, dtype=np.int32); hits = np.zeros(9, dtype=np.int32)
        args = (L._ip(samples), L._ip(hits), None, None)
        assert eng.lib.mvicp_overlap(eng.h, L._dp(P), C.c_float(0.05), 0, *args) == -3          # mvicp_set_num_frames not called
        eng.lib.mvicp_set_num_frames(eng.h, 3)
        eng.n_frames = 3; eng.npts = [0, 0, 0]
        eng.set_frame(0, pb["pts"][0]); eng.set_frame(1, pb["pts"][1])
        assert eng.lib.mvicp_overlap(eng.h, L._dp(P), C.c_float(0.05), 0, *args) == -3          # frame 2 never uploaded
        assert b"frame 2" in eng.lib.mvicp_last_error()
        eng.set_frame(2, pb["pts"][2])
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert eng.lib.mvicp_overlap(eng.h, L._dp(P), C.c_float(bad), 0, *args) == -1, bad
        Pn = P.copy(); Pn[1, 13] = np.nan
        assert eng.lib.mvicp_overlap(eng.h, L._dp(Pn), C.c_float(0.05), 0, *args) == -1
        assert eng.lib.mvicp_overlap(eng.h, None, C.c_float(0.05), 0, *args) == -1
        assert eng.lib.mvicp_overlap(eng.h, L._dp(P), C.c_float(0.05), 0, None, L._ip(hits), None, None) == -1
        assert eng.lib.mvicp_overlap(eng.h, L._dp(P), C.c_float(0.05), 0, L._ip(samples), None, None, None) == -1
        got = eng.overlap(pb["init"], 0.05, 0)                 # still works; sumq / q_exp may be NULL
        assert eng.lib.mvicp_overlap(eng.h, L._dp(P), C.c_float(0.05), 0, *args) == 0
        assert np.array_equal(hits.reshape(3, 3), got["hits"]) and got["hits"][1, 0] > 0
        eng.set_graph(pb["src"], pb["dst"])
        counts, _ = eng.correspond(pb["init"], pb["fixed"], 0.05)
        for e, (s, d) in enumerate(zip(pb["src"], pb["dst"])):  # hits == counts of the search with the same cutoff
            assert counts[e] == eng.overlap(pb["init"], 0.05, 0)["hits"][s, d]
    finally:
        eng.close()
