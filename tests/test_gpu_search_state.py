"""-m gpu: a search is a pure function of (clouds, graph, poses, fixed mask, cutoff, tie rule) — also after a search that FAILED and after a
flip of the "tie_rule" option.

mvicp_correspond keeps a dozen cross-round fields (the table above correspond_once in csrc/api.cpp).  Two ways to leave them describing a
search that never happened:

  A. a search that fails after its per-edge loop (an unknown nn_method, an injected / real launch failure) has already overwritten
     prev_xf / prev_q with the transforms of the failed call, while seeds, bounds, lists and cache flags still belong to the last search
     that succeeded.  A retry at the poses of the failed call then looks bit-identical to "last search" and may hand out the OLD lists (with the
     grid kernel: no compaction, no gather; after an argument error the epochs are kept as well); a retry at a third pose computes its cache
     displacement from the failed pose.
  B. "tie_rule" decides which of several equidistant targets a query gets, but changing it invalidated nothing: the next search at
     bit-identical poses kept epochs, the exported copy and the lists of the other rule.

Every search of the sequences below is compared with FRESH contexts asked once at the same poses (one with NN_BRUTE, one with NN_AUTO; counts,
weight bytes, offsets and the full triples of map_correspondences), which in turn are held to the oracle on one edge; the tie-rule cases
also to the real nanoflann through tests/cpupath.py.  The fresh answers are computed once per module and shared."""
import numpy as np
import pytest

import cpupath
import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
CUTOFF = 0.05
METHODS = {"grid": L.NN_GRID, "tile": L.NN_TILE, "auto": L.NN_AUTO, "brute": L.NN_BRUTE}


def fresh(pts, nor, src, dst, poses, fixed, method, tie_rule=1):
    """-> (counts, weight bytes, offsets, triples) of a context that has never searched before."""
    B = mvicp.Engine(0)
    try:
        B.set_option("tie_rule", tie_rule)
        B.set_frames(pts, nor); B.set_graph(src, dst)
        c, w = B.correspond(poses, fixed, CUTOFF, method)
        t, o = B.map_correspondences()
        return c.copy(), w.tobytes(), o.copy(), t.copy()
    finally:
        B.close()


def assert_same(got, want, tag):
    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (tag, "counts / weights", got[0], want[0])
    assert np.array_equal(got[2], want[2]), (tag, "offsets")
    bad = int((got[3] != want[3]).sum())
    assert bad == 0, (tag, f"{bad} of {len(want[3])} triples differ from a fresh context")


def search(A, poses, fixed, method):
    c, w = A.correspond(poses, fixed, CUTOFF, method)
    t, o = A.map_correspondences()
    return c.copy(), w.tobytes(), o.copy(), t.copy()


def second_changed(a, b, e):
    """fraction of the sources edge e has in both results whose `second` differs"""
    ta, tb = a[3][a[2][e]:a[2][e + 1]], b[3][b[2][e]:b[2][e + 1]]
    common, ia, ib = np.intersect1d(ta["first"], tb["first"], return_indices=True)
    assert len(common) > 100
    return float((ta["second"][ia] != tb["second"][ib]).mean())


# ---------------------------------------------------------------- A. searches after a failed call
@pytest.fixture(scope="module")
def world(orc):
    pb = synth.make_problem(3, 3000)
    fixed = pb["fixed"]
    P0 = pb["gt"].copy()
    P1 = P0.copy()
    free = [k for k in range(3) if not fixed[k]]
    for k in free:
        P1[k][:3, 3] += 3e-3 * np.array([1.0, -0.5, 0.25]) * (1.0 if k % 2 else -1.0)
    P2 = P1.copy(); P2[free[0]][0, 3] += 1e-6
    poses = {"P0": P0, "P1": P1, "P2": P2}
    ref = {}
    for e_chk, (name, P) in enumerate(poses.items()):
        rb = fresh(pb["pts"], pb["nor"], pb["src"], pb["dst"], P, fixed, L.NN_BRUTE)
        ra = fresh(pb["pts"], pb["nor"], pb["src"], pb["dst"], P, fixed, L.NN_AUTO)
        assert_same(ra, rb, ("fresh AUTO vs fresh BRUTE", name))
        active = [e for e, s in enumerate(pb["src"]) if not fixed[s]]
        e = active[e_chk % len(active)]                       # ... and the oracle on one edge
        s, d = pb["src"][e], pb["dst"][e]
        f, sec, dist, w, _, _ = orc.correspond_edge(pb["pts"][s], P[s], pb["pts"][d], P[d], CUTOFF)
        t = rb[3][rb[2][e]:rb[2][e + 1]]
        assert np.array_equal(t["first"], f) and np.array_equal(t["second"], sec) and t["dist"].tobytes() == dist.tobytes(), (name, e)
        assert np.frombuffer(rb[1], dtype=np.float32)[e] == w
        ref[name] = rb
    active = [e for e, s in enumerate(pb["src"]) if not fixed[s]]
    # input condition, from fresh contexts alone: the step P0 -> P1 really changes the lists (a stale list would not go unnoticed)
    moved = [second_changed(ref["P0"], ref["P1"], e) for e in active]
    print("P0 -> P1: `second` changes for", ["%.0f %%" % (100 * m) for m in moved], "of the common sources on edges", active)
    assert min(moved) >= 0.25, moved
    assert not np.array_equal(ref["P1"][3], ref["P2"][3]) or ref["P1"][1] != ref["P2"][1]   # (P2 is not P1 either: the distances moved)
    return {"pb": pb, "fixed": fixed, "poses": poses, "ref": ref, "active": active}


@pytest.mark.parametrize("variant", ["plain", "optimize", "retry_at_p2"])
@pytest.mark.parametrize("failure", ["fault_inject", "nn_method_99"])
@pytest.mark.parametrize("method", list(METHODS))
def test_searches_after_a_failed_call_equal_a_fresh_context(world, method, failure, variant):
    pb, fixed, poses, ref, active = world["pb"], world["fixed"], world["poses"], world["ref"], world["active"]
    m = METHODS[method]
    A = mvicp.Engine(0)
    try:
        A.set_frames(pb["pts"], pb["nor"]); A.set_graph(pb["src"], pb["dst"])

        def step(name, tag):
            got = search(A, poses[name], fixed, m)
            assert_same(got, ref[name], (method, failure, variant, tag))
            if variant == "optimize":                          # a solve after every search: the next search queues its first evaluation
                A.optimize(poses[name], fixed, L.PARAM_SOPHUS_SE3, 1, True, 50)

        for r in range(3):                                     # caches, lists and the fixed-point shortcuts are live
            step("P0", f"warm-up {r}")
        ep0 = A.correspondence_epochs()
        if failure == "fault_inject":
            A.set_option("fault_inject", 1)
        with pytest.raises(mvicp.MvicpError):
            A.correspond(poses["P1"], fixed, CUTOFF, 99 if failure == "nn_method_99" else m)
        if variant == "retry_at_p2":
            step("P2", "retry at a third pose")
            ep = A.correspondence_epochs()
            assert all(ep[e] != ep0[e] for e in active), (ep0, ep)
            step("P2", "again")
            assert np.array_equal(A.correspondence_epochs(), ep)
            step("P0", "back")
            return
        step("P1", "retry at the failed call's poses")
        ep1 = A.correspondence_epochs()
        assert all(ep1[e] != ep0[e] for e in active), (ep0, ep1)   # a failed search gives every edge a new, never repeated epoch
        assert len(set(ep1[active].tolist()) & set(ep0.tolist())) == 0
        step("P1", "again")
        assert np.array_equal(A.correspondence_epochs(), ep1)       # bit-identical inputs: every epoch is kept
        step("P2", "a third pose")
        step("P0", "back")
    finally:
        A.close()


# ---------------------------------------------------------------- B. the tie rule is an input
@pytest.fixture(scope="module")
def dup_world(orc, refnn):
    """The recipe of test_gpu_parity.py::test_duplicate_targets_through_the_correspondence_path: a third of every cloud exists twice."""
    assert refnn is not None, "oracle/_ref (real nanoflann) was not built"
    pb = synth.make_problem(3, 3000)
    rng = np.random.default_rng(11)
    pts = [p.copy() for p in pb["pts"]]; nor = [n.copy() for n in pb["nor"]]
    for k in range(3):
        pick = rng.choice(len(pts[k]), len(pts[k]) // 3, replace=False)
        pts[k] = np.vstack([pts[k], pts[k][pick]]); nor[k] = np.vstack([nor[k], nor[k][pick]])
    P0 = pb["gt"].copy()
    ref = {}
    for rule in (0, 1):
        rb = fresh(pts, nor, pb["src"], pb["dst"], P0, pb["fixed"], L.NN_BRUTE, rule)
        ra = fresh(pts, nor, pb["src"], pb["dst"], P0, pb["fixed"], L.NN_AUTO, rule)
        assert_same(ra, rb, ("fresh AUTO vs fresh BRUTE, rule", rule))
        ref[rule] = rb
    # rule 1 is the real nanoflann's answer, rule 0 the oracle's lowest index
    cpu = cpupath.CpuPath(pts, nor, pb["src"], pb["dst"], pb["fixed"], 2, 1, orc=orc, ref=refnn)
    nano = cpu.correspond(P0)
    cpu.close()
    differ = []
    for e in range(len(pb["src"])):
        t1 = ref[1][3][ref[1][2][e]:ref[1][2][e + 1]]
        f, s2, d, w = nano[e]
        assert np.array_equal(t1["first"], f) and np.array_equal(t1["second"], s2) and t1["dist"].tobytes() == d.tobytes(), e
        t0 = ref[0][3][ref[0][2][e]:ref[0][2][e + 1]]
        if len(f):
            lo = orc.correspond_edge(pts[pb["src"][e]], P0[pb["src"][e]], pts[pb["dst"][e]], P0[pb["dst"][e]], CUTOFF)[1]
            assert np.array_equal(t0["second"], lo), e
        if not np.array_equal(t0, t1):
            differ.append(e)
    n_diff = int((ref[0][3]["second"] != ref[1][3]["second"]).sum()) if len(ref[0][3]) == len(ref[1][3]) else -1
    print("tie rule 1 vs 0 at P0: lists differ on edges", differ, "-", n_diff, "of", len(ref[1][3]), "`second` entries")
    assert differ, "the data must make the two tie rules disagree somewhere"   # input condition, from fresh contexts alone
    return {"pb": pb, "pts": pts, "nor": nor, "P0": P0, "ref": ref, "differ": differ}


@pytest.mark.parametrize("first_rule", [1, 0])
@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("method", ["grid", "tile", "auto"])
def test_a_tie_rule_flip_at_identical_poses_changes_the_lists(dup_world, method, lazy, first_rule):
    D = dup_world
    pb, P0, ref = D["pb"], D["P0"], D["ref"]
    m = METHODS[method]
    A = mvicp.Engine(0)
    try:
        A.set_option("tie_lazy", lazy)
        A.set_option("tie_rule", first_rule)
        A.set_frames(D["pts"], D["nor"]); A.set_graph(pb["src"], pb["dst"])
        for r in range(2):
            assert_same(search(A, P0, pb["fixed"], m), ref[first_rule], (method, lazy, first_rule, f"first rule, search {r}"))
        ep0 = A.correspondence_epochs()
        A.set_option("tie_rule", 1 - first_rule)
        assert_same(search(A, P0, pb["fixed"], m), ref[1 - first_rule], (method, lazy, first_rule, "after the flip"))
        ep1 = A.correspondence_epochs()
        assert all(ep1[e] != ep0[e] for e in D["differ"]), (ep0, ep1, D["differ"])
        assert_same(search(A, P0, pb["fixed"], m), ref[1 - first_rule], (method, lazy, first_rule, "after the flip, again"))
        assert np.array_equal(A.correspondence_epochs(), ep1)
        A.set_option("tie_rule", 1 - first_rule)               # setting the value it has changes nothing
        assert_same(search(A, P0, pb["fixed"], m), ref[1 - first_rule], (method, lazy, first_rule, "same value set again"))
        assert np.array_equal(A.correspondence_epochs(), ep1)
        A.set_option("tie_rule", first_rule)
        assert_same(search(A, P0, pb["fixed"], m), ref[first_rule], (method, lazy, first_rule, "flipped back"))
        ep2 = A.correspondence_epochs()
        assert all(ep2[e] != ep1[e] and ep2[e] != ep0[e] for e in D["differ"]), (ep0, ep1, ep2)
    finally:
        A.close()


# ---------------------------------------------------------------- failures and rule flips among the other regime events
@pytest.mark.parametrize("seed", range(4))
def test_regime_transitions_with_failed_searches_and_tie_rule_flips(dup_world, orc, seed):
    """tests/test_gpu_parity.py::test_correspond_regime_transitions_match_a_fresh_context with two more events — "fail" (an injected launch
    failure or an unknown nn_method, at poses of its own) and "tie_rule" — on clouds with duplicated points, where the rule matters.  (A
    generator of its own with seeds of its own: the sequences that test draws stay what they are.)"""
    D = dup_world
    pb, pts, nor = D["pb"], D["pts"], D["nor"]
    src, dst = pb["src"], pb["dst"]
    rng = np.random.default_rng(9100 + seed)
    A = mvicp.Engine(0)
    try:
        A.set_frames(pts, nor); A.set_graph(src, dst)
        poses = pb["init"].copy()
        fixed = pb["fixed"].copy()
        cutoff, method, rule = CUTOFF, L.NN_AUTO, 1
        events = []
        for rnd in range(12):
            ev = str(rng.choice(["none", "fail", "fail", "tie_rule", "tie_rule", "hold", "hold", "method", "cutoff", "reset", "option"])) if rnd > 0 else "none"
            events.append(ev)
            if ev == "cutoff":
                cutoff = float(rng.choice([0.05, 0.02, 0.008]))
            elif ev == "reset":
                A.reset_history()
            elif ev == "method":
                method = int(rng.choice([L.NN_AUTO, L.NN_BRUTE, L.NN_GRID, L.NN_TILE]))
            elif ev == "option":
                A.set_option(str(rng.choice(["list_reuse", "nn_cache", "sel_bracket", "spec_eval", "tile_cache"])), float(rng.integers(0, 2)))
            elif ev == "tie_rule":
                rule = 1 - rule
                A.set_option("tie_rule", rule)
            elif ev == "fail":
                Pf = poses.copy()
                Pf[1 + int(rng.integers(0, 2))][:3, 3] += rng.normal(0.0, 2e-3, 3)
                bad_arg = bool(rng.integers(0, 2))
                if not bad_arg:
                    A.set_option("fault_inject", 1)
                with pytest.raises(mvicp.MvicpError):
                    A.correspond(Pf, fixed, np.float32(cutoff), 99 if bad_arg else method)
                if rng.random() < 0.5:
                    poses = Pf                                 # the retry at the failed call's poses; else at the poses before it
            counts, weights = A.correspond(poses, fixed, cutoff, method)
            trip, off = A.map_correspondences()
            B = mvicp.Engine(0)
            try:
                B.set_option("tie_rule", rule)
                B.set_frames(pts, nor); B.set_graph(src, dst)
                cb, wb = B.correspond(poses, fixed, cutoff, L.NN_BRUTE if rnd % 2 == 0 else L.NN_AUTO)
                tb, ob = B.map_correspondences()
            finally:
                B.close()
            assert np.array_equal(counts, cb) and weights.tobytes() == wb.tobytes(), (seed, rnd, events)
            assert np.array_equal(off, ob) and np.array_equal(trip, tb), (seed, rnd, events, int((trip != tb).sum()) if len(trip) == len(tb) else -1)
            if rule == 0:
                e = int(rng.integers(0, len(src)))
                if not fixed[src[e]]:
                    f, sec, dist, w, _, _ = orc.correspond_edge(pts[src[e]], poses[src[e]], pts[dst[e]], poses[dst[e]], cutoff)
                    t = trip[off[e]:off[e + 1]]
                    assert np.array_equal(t["first"], f) and np.array_equal(t["second"], sec) and t["dist"].tobytes() == dist.tobytes() and weights[e] == w, (seed, rnd, e, events)
            if ev not in ("hold", "fail") and counts.sum() > 0:
                poses, sm = A.optimize(poses, fixed, int(rng.integers(0, 3)), int(rng.integers(0, 2)), bool(rng.integers(0, 2)), 50)
    finally:
        A.close()
