"""-m gpu: the median of the accepted d2 per edge (corr.hip): the two-pass select anchored at the acceptance bound — histogram of an anchored
2048-bin digit -> pick of the median's bin -> count / compact / select inside the bin — and the searches that launch no select at all because no
list can change (option sel_reuse).  Every count and weight is compared bit for bit with the host rule (frame.cpp:156-176): np.partition at
size // 2, x 1.5, to float32."""
import numpy as np
import pytest

import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def _weight_ref(d2, thresh):
    """frame.cpp:156-176 on the host: keep sqrt(d2) < (double)thresh, upper median, x1.5, to float."""
    d = np.sqrt(d2)
    d = d[d < float(np.float32(thresh))]
    if d.size == 0:
        return 0, np.float32(0)
    return d.size, np.float32(np.partition(d, d.size // 2)[d.size // 2] * 1.5)


# ---------------------------------------------------------------- 1. key sets that stress each stage

# case -> (cutoff, offsets of the n sources from their targets).  With the cutoff 0.05 the bound on d2 is 2.5e-3: bin 2047 of the anchored digit
# starts 1.1 % below it, bin 0 ends 32 octaves below it (5.8e-13).
def _offsets(case, n, rng):
    x = np.array([[1.0, 0.0, 0.0]])
    if case == "all_zero":               # one key value: the picked bin is the whole list (bin 0)
        return 0.05, np.zeros((n, 3))
    if case == "low_bits":               # d2 ~ 9e-10 for every pair: the keys differ only through the rounding of x + 3e-5
        return 0.05, np.tile([3e-5, 0.0, 0.0], (n, 1))
    if case == "top_bin":                # just inside the cutoff: d2 within 2e-4 (relative) of the bound, all in bin 2047
        return 0.05, 0.05 * (1.0 - 1e-4 * rng.uniform(0.01, 1.0, (n, 1))) * x
    if case == "wide":                   # d2 from 1e-30 to just under the bound: the median (d2 ~ 5e-17) lies in the shared bin 0
        return 0.05, (10.0 ** rng.uniform(-15.0, np.log10(0.0499), (n, 1))) * x
    if case == "huge_cutoff":            # bound 1e6, d2 ~ 1e-10: every key in bin 0, the finish selects among all n keys (global-memory path beyond 2048)
        return 1e3, 1e-5 * rng.uniform(0.5, 1.5, (n, 1)) * x
    assert case == "none_accepted"       # count = 0
    return 1e-9, np.tile([1e-4, 0.0, 0.0], (n, 1))


def _bins(d2, thresh):
    """The anchored digit of DESIGN.md section 3.4 for the accepted keys: clamp(2047 - ((kb >> 46) - (key >> 46)), 0, 2047), kb = the pattern of the
    d2 acceptance bound (the smallest double whose sqrt is >= the cutoff).  Only used to check that a case puts its keys where its name says."""
    t = float(np.float32(thresh))
    bound = t * t
    while np.sqrt(bound) >= t:
        bound = np.nextafter(bound, 0.0)
    while np.sqrt(bound) < t:
        bound = np.nextafter(bound, np.inf)
    kb = int(np.float64(bound).view(np.int64))
    keys = d2[np.sqrt(d2) < t].view(np.int64)
    return np.clip(2047 - ((kb >> 46) - (keys >> 46)), 0, 2047)


@pytest.mark.parametrize("n", [1, 2, 3, 9001, 20_001])   # kSelBlock = 8192: 1, 2 and 3 select workgroups; 20 001 has an odd count
@pytest.mark.parametrize("case", ["all_zero", "low_bits", "top_bin", "wide", "huge_cutoff", "none_accepted"])
def test_anchored_select_on_key_sets_that_stress_each_stage(eng, case, n):
    rng = np.random.default_rng(11)
    dst = rng.uniform(-4.0, 4.0, (n, 3))
    thresh, off = _offsets(case, n, rng)
    src = dst + off
    I = np.eye(4)
    poses = np.stack([I, I])
    fixed = np.array([1, 0], dtype=np.uint8)
    eng.set_frames([dst, src], [None, None]); eng.set_graph([1], [0])
    idx, d2 = eng.nn_query(0, src, L.NN_BRUTE)
    want_n, want_w = _weight_ref(d2, thresh)
    if case == "none_accepted":
        assert want_n == 0
    elif case != "wide":
        assert want_n == n
    b = _bins(d2, thresh)
    if case in ("all_zero", "huge_cutoff"):
        assert np.all(b == 0)
    elif case == "top_bin":
        assert np.mean(b == 2047) > 0.9 and np.partition(b, b.size // 2)[b.size // 2] == 2047   # (a few sources have a nearer target than their own)
    elif case == "wide":
        assert np.partition(b, b.size // 2)[b.size // 2] == 0 and (n < 100 or b.max() > 1500)
    for method in (L.NN_GRID, L.NN_TILE):
        counts, weights = eng.correspond(poses, fixed, thresh, method)
        assert counts[0] == want_n, (case, n, method)
        assert weights.dtype == np.float32 and weights[0].tobytes() == want_w.tobytes(), (case, n, method, weights[0], want_w)


# ---------------------------------------------------------------- 2./3. several edges, and the searches without a select

def _problem():
    """3 views x 800 points.  View 1 is rebuilt as view 0's points seen from view 1 plus 1e-7 of noise, so the edge 1 -> 0 has d2 ~ 1e-14 where
    the other edges have the sampling distance of the surface (d2 ~ 1e-4 ... 1e-3): medians orders of magnitude apart in one launch."""
    pb = synth.make_problem(3, 800)
    rng = np.random.default_rng(5)
    T0, T1 = pb["gt"][0], pb["gt"][1]
    world = pb["pts"][0] @ T0[:3, :3].T + T0[:3, 3]
    pb["pts"][1] = np.ascontiguousarray((world - T1[:3, 3]) @ T1[:3, :3] + rng.normal(0, 1e-7, world.shape))
    pb["nor"][1] = np.ascontiguousarray(pb["nor"][0] @ T0[:3, :3].T @ T1[:3, :3])
    return pb


@pytest.fixture(scope="module")
def pb3():
    return _problem()


def _host_rule(orc, pb, poses, fixed, thresh):
    counts, weights = [], []
    for s, d in zip(pb["src"], pb["dst"]):
        if fixed[s]:
            counts.append(0); weights.append(np.float32(0)); continue
        nn_d2 = orc.correspond_edge(pb["pts"][s], poses[s], pb["pts"][d], poses[d], thresh)[5]
        n, w = _weight_ref(nn_d2, thresh)
        counts.append(n); weights.append(w)
    return np.array(counts), np.array(weights, dtype=np.float32)


@pytest.mark.parametrize("method", [L.NN_GRID, L.NN_TILE, L.NN_AUTO])
def test_edges_with_different_distributions_in_one_launch(orc, pb3, method):
    fixed = np.array([1, 0, 1], dtype=np.uint8)       # the edges out of view 2 are inactive
    e = mvicp.Engine(0)
    try:
        e.set_frames(pb3["pts"], pb3["nor"]); e.set_graph(pb3["src"], pb3["dst"])
        want_c, want_w = _host_rule(orc, pb3, pb3["gt"], fixed, 0.05)
        act = want_w[want_c > 0].astype(np.float64)
        assert act.size >= 2 and act.max() > 100.0 * act.min(), want_w
        assert any(fixed[s] for s in pb3["src"])
        for _ in range(2):
            c, w = e.correspond(pb3["gt"], fixed, 0.05, method)
            assert np.array_equal(c, want_c) and w.tobytes() == want_w.tobytes(), (c, want_c, w, want_w)
        free = np.array([1, 0, 0], dtype=np.uint8)    # every edge active, each with its own median
        want_c, want_w = _host_rule(orc, pb3, pb3["gt"], free, 0.05)
        c, w = e.correspond(pb3["gt"], free, 0.05, method)
        assert np.array_equal(c, want_c) and w.tobytes() == want_w.tobytes(), (c, want_c, w, want_w)
    finally:
        e.close()


def test_no_select_launch_while_no_list_can_change(orc, pb3):
    fixed = np.array([1, 0, 0], dtype=np.uint8)
    P = pb3["gt"].copy()
    e = mvicp.Engine(0)
    try:
        e.set_frames(pb3["pts"], pb3["nor"]); e.set_graph(pb3["src"], pb3["dst"])
        e.profile(1)
        sel = lambda: e.profile_get("select")[1]
        hit = lambda: e.profile_get("spec.hit")[1]

        def search(poses, fx, thresh, grows):
            before = sel()
            c, w = e.correspond(poses, fx, thresh, L.NN_GRID)
            assert (sel() > before) == grows, (sel(), before, grows)
            want_c, want_w = _host_rule(orc, pb3, poses, fx, thresh)
            assert np.array_equal(c, want_c) and w.tobytes() == want_w.tobytes(), (c, want_c, w, want_w)
            return c, w

        c0, w0 = search(P, fixed, 0.05, True)
        for _ in range(2):                                   # same poses: no select, same bytes
            c, w = search(P, fixed, 0.05, False)
            assert np.array_equal(c, c0) and w.tobytes() == w0.tobytes()
        P1, sm1 = e.optimize(P, fixed, L.PARAM_SOPHUS_SE3, True, True, 50)   # the first solve: from now on a search queues the next solve's first evaluation
        # ... whose SoftLOne scales the last select did not write on the device: this one search launches the select again, the next ones do not
        search(P, fixed, 0.05, True)
        search(P, fixed, 0.05, False)
        h = hit()
        P1b, sm1b = e.optimize(P, fixed, L.PARAM_SOPHUS_SE3, True, True, 50)
        assert hit() == h + 1                                # served by the evaluation queued in a search without a select
        assert P1b.tobytes() == P1.tobytes() and sm1b == sm1
        search(P, fixed, 0.05, False)
        # everything that can change a list, or the select's result on the device, brings the select back — once
        P2 = P.copy(); P2[1][0, 3] += 1e-6
        search(P2, fixed, 0.05, True)
        search(P2, fixed, 0.05, False)
        search(P2, fixed, 0.04, True)                        # the cutoff
        search(P2, fixed, 0.04, False)
        fixed2 = np.array([1, 0, 1], dtype=np.uint8)
        search(P2, fixed2, 0.04, True)                       # a fixed flag
        search(P2, fixed2, 0.04, False)
        e.reset_history()
        search(P2, fixed2, 0.04, True)
        search(P2, fixed2, 0.04, False)
        edge = next(k for k, s in enumerate(pb3["src"]) if not fixed2[s])
        ids = np.arange(5, dtype=np.int32)
        e.set_correspondences(edge, ids, ids, 0.25)
        search(P2, fixed2, 0.04, True)
        search(P2, fixed2, 0.04, False)
        e.set_option("sel_reuse", 0)
        search(P2, fixed2, 0.04, True)
        search(P2, fixed2, 0.04, True)
        e.set_option("sel_reuse", 1)
        search(P2, fixed2, 0.04, False)
        e.set_option("fault_inject", 1)
        with pytest.raises(mvicp.MvicpError):
            e.correspond(P2, fixed2, 0.04, L.NN_GRID)
        search(P2, fixed2, 0.04, True)                       # a failed search leaves nothing to reuse
        search(P2, fixed2, 0.04, False)
    finally:
        e.close()


# ---------------------------------------------------------------- 4. trajectory

def test_trajectory_is_the_same_with_and_without_select_reuse():
    pb = synth.make_problem(4, 20_000)
    res = {}
    for reuse in (1, 0):
        e = mvicp.Engine(0)
        try:
            e.set_option("sel_reuse", reuse)
            e.set_frames(pb["pts"], pb["nor"]); e.set_graph(pb["src"], pb["dst"])
            e.profile(True)
            poses = pb["init"].copy()
            log = []
            for r in range(16):
                e.profile_reset()
                c, w = e.correspond(poses, pb["fixed"], 0.05)
                nsel = e.profile_get("select")[1]
                poses, sm = e.optimize(poses, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
                log.append((c.copy(), w.tobytes(), poses.copy(), sm, nsel))
            res[reuse] = log
        finally:
            e.close()
    for r, (a, b) in enumerate(zip(res[1], res[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], r
        assert a[2].tobytes() == b[2].tobytes(), r
        assert a[3] == b[3], (r, a[3], b[3])
    assert all(l[4] >= 1 for l in res[0]), [l[4] for l in res[0]]        # sel_reuse = 0: every search launches its select
    skipped = [l[4] == 0 for l in res[1]]
    assert any(skipped) and not skipped[0], skipped                  # some rounds of the converged registration launched none
