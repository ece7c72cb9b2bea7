"""The search policy of mvicp_correspond (mv-lm-icp_amd/csrc/search_plan.h: plan_search, record_queued, record_arrived) without a GPU.

tests/plan_harness.cpp is compiled with g++ and driven through ctypes.  The graph is 3 frames and 4 edges (0->1, 1->0, 1->2, 2->1; frame 0
fixed, so edge 0 is never searched); the clouds exist only as (n, max_norm, cell, flags) = (100 / 200 / 300 points, 1.0, 0.1, ...).  What a
round observes — counts, median d2, the tie and far words — is fed in by the test.  Every expected plan is written out by hand from the
documented rules (the bracket 0.994 / 1.006 within 0.1 %, AUTO's 1.5 x cell and 0.5 x cell, the option defaults), never computed by the
planner, and every assertion compares a whole plan: all its graph-wide fields, or all per-edge rows.

A poses argument p(x1, y2) below means: frame 1 translated by x1 along x, frame 2 by y2 along y, rotations the identity — so dM = 0 and
every active edge's queries move by exactly |change of x1| (edges 1, 2) or of (x1, y2) (edge 3) between two searches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mv-lm-icp_amd", "csrc")
AUTO, BRUTE, GRID, TILE = 0, 1, 2, 3
ERR_ARG = -1
SRC, DST = [0, 1, 1, 2], [1, 0, 2, 1]
NPTS = [100, 200, 300]
CELL = 0.1
FIXED = [1, 0, 0]
CUTOFF = 0.05


class PlanOut(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("status", "method", "tile_lb", "tile_cached", "handed_over", "cached_on_mfma", "all_same", "same_active_set",
                                      "all_unchanged", "nothing_can_change", "tie_skip", "far_skip", "far_narrow", "tie_launched", "far_launched",
                                      "sel_skip", "use_bracket", "spec_arm", "spec2_plan", "n_tie_need")] + [("eps_over_mu", C.c_double)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plan") / "plan_harness.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tests", "plan_harness.cpp")], timeout=300)
    L = C.CDLL(so)
    L.plan_new.restype = C.c_void_p
    L.plan_new.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.plan_free.argtypes = [C.c_void_p]
    L.plan_set_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int]
    L.plan_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    L.plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(PlanOut)]
    L.plan_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.plan_queued.argtypes = [C.c_void_p]
    L.plan_arrived.argtypes = [C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p, C.c_int]
    L.plan_forget.argtypes = [C.c_void_p]
    L.plan_explicit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.plan_solved.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.plan_candidate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.plan_history.argtypes = [C.c_void_p, C.c_void_p]
    return L


def p(x1, y2=0.0):
    P = np.tile(np.eye(4), (3, 1, 1))
    P[1][0, 3] = x1
    P[2][1, 3] = y2
    return np.ascontiguousarray(P.transpose(0, 2, 1).reshape(3, 16))    # column-major 4 x 4 per frame


class Planner:
    """One context's worth of policy state.  frame_flags: 1 grid structures, 2 tie tree, 4 sorted normals."""
    def __init__(self, lib, frame_flags=(5, 5, 5), exchange=0, world=1, owned=(1, 1, 1, 1), **options):
        self.L, self.exchange, self.world = lib, exchange, world
        src, dst, own = np.array(SRC, np.int32), np.array(DST, np.int32), np.array(owned, np.uint8)
        self.h = lib.plan_new(3, 4, src.ctypes.data, dst.ctypes.data, own.ctypes.data)
        for k in range(3):
            lib.plan_set_frame(self.h, k, NPTS[k], 1.0, CELL, frame_flags[k])
        for name, v in options.items():
            self.option(name, v)
        self.spec_arm = 0

    def option(self, name, v):
        assert self.L.plan_set_option(self.h, name.encode(), float(v)) == 0, name

    def plan(self, poses, fixed=FIXED, cutoff=CUTOFF, method=AUTO):
        """-> (graph-wide fields as a dict, per-edge rows, frames that need a tie tree).  A row is (active, src_fixed, nsrc, same_edge,
        unchanged, dirty, cache slot class, lo, hi); the class of the cache slot is -1 (no cache), 0 (bit-identical) or 1 (an allowance > 0)."""
        out = PlanOut()
        fx = np.array(fixed, np.uint8)
        st = self.L.plan_run(self.h, poses.ctypes.data, fx.ctypes.data, cutoff, method, self.exchange, self.world, C.byref(out))
        assert st == out.status
        ints, reals, need = np.zeros((4, 6), np.int32), np.zeros((4, 3)), np.zeros(8, np.int32)
        self.L.plan_rows(self.h, ints.ctypes.data, reals.ctypes.data, need.ctypes.data)
        g = {n: getattr(out, n) for n, _ in PlanOut._fields_}
        g["eps_over_mu"] = round(g["eps_over_mu"], 6)
        rows = [tuple(int(v) for v in ints[e]) + (int(np.sign(reals[e, 0])), float(reals[e, 1]), float(reals[e, 2])) for e in range(4)]
        self.spec_arm = out.spec_arm
        self.active = [int(ints[e, 0]) for e in range(4)]
        if self.exchange:      # the exchanged buffer holds every rank's searched edges
            self.active = [int(not ints[e, 1]) for e in range(4)]
        return g, rows, [int(v) for v in need[:out.n_tie_need]]

    def finish(self, d, tie=0, far=0, armed=None, redone=0):
        """The rest of the round: the NN launch is queued, then (count, median d2 = d^2) arrive for the searched edges (d: one distance or one
        per edge), with the tie / far words and the armed slot (default: what this rank's plan armed)."""
        d = [d] * 4 if np.isscalar(d) else d
        self.L.plan_queued(self.h)
        res = np.zeros(9)
        for e in range(4):
            if self.active[e]:
                res[2 * e], res[2 * e + 1] = NPTS[SRC[e]] // 2, d[e] * d[e]
        res[8] = float(self.spec_arm * self.world) if armed is None else armed
        scales = np.array([float(np.float32(np.sqrt(res[2 * e + 1]) * 1.5)) for e in range(4)])
        return self.L.plan_arrived(self.h, tie, far, res.ctypes.data, scales.ctypes.data, redone)

    def round(self, poses, d, **kw):
        out = self.plan(poses, **kw)
        self.finish(d)
        return out

    def history(self):
        out = np.zeros(6, np.int32)
        self.L.plan_history(self.h, out.ctypes.data)
        return dict(zip(("auto_last_method", "nn_cache_valid", "sel_result_valid", "sel_result_armed", "corr_tie_seen", "corr_far_seen"), (int(v) for v in out)))

    def close(self):
        self.L.plan_free(self.h)


def G(**kw):
    """a plan's graph-wide fields: a first search's, with the given ones changed"""
    g = dict(status=0, method=TILE, tile_lb=0, tile_cached=0, handed_over=0, cached_on_mfma=0, all_same=0, same_active_set=0, all_unchanged=0,
             nothing_can_change=0, tie_skip=0, far_skip=0, far_narrow=0, tie_launched=1, far_launched=0, sel_skip=0, use_bracket=0, spec_arm=0,
             spec2_plan=0, n_tie_need=0, eps_over_mu=-1.0)
    assert set(kw) <= set(g)
    g.update(kw)
    return g


def row(t, n):
    """a row given without its nsrc column, for a source of n points"""
    return t[:2] + (n if t[0] else 0,) + t[2:]


def rows(e0, e12, e3=None):
    """edge 0's row (complete), the rows of edges 1 and 2 (sources of 200 points) and of edge 3 (300 points; default: like edges 1 and 2)"""
    return [e0, row(e12, 200), row(e12, 200), row(e3 or e12, 300)]


# the rows that recur.  (active, src_fixed, [nsrc: E0_* only,] same_edge, unchanged, dirty, cache class, lo, hi)
E0_FIRST = (0, 1, 0, 0, 0, 1, -1, 0.0, 0.0)          # the fixed frame's edge in a first search
E0_KEPT = (0, 1, 0, 0, 1, 1, -1, 0.0, 0.0)           # ... later: not searched then, not searched now, empty: unchanged
A_FIRST = (1, 0, 0, 0, 1, -1, 0.0, 0.0)              # searched, no history: no cache, list rebuilt
A_MOVED = (1, 0, 0, 0, 0, -1, 0.0, 0.0)              # searched before, transform moved, no bounds from last round: list kept, no cache
A_CACHED = (1, 0, 0, 0, 0, 1, 0.0, 0.0)              # ... with bounds from last round: the cache is on with an allowance
A_SAME = (1, 0, 1, 1, 0, 0, 0.0, 0.0)                # bit-identical transform: allowance 0, list unchanged


def to_hand_over(P):
    """rounds 1-4 of a registration whose median distance goes 0.2, 0.09, 0.08 (cell 0.1).  -> the four plans"""
    return [P.round(p(0.30), 0.2), P.round(p(0.20), 0.09), P.round(p(0.12), 0.08), P.round(p(0.11), 0.079)]


def to_fixed_point(P, tie=0, far=0):
    """... then a cache-aware round (which reports `tie`) and the first round at bit-identical poses (which reports `tie` and `far`, where it
    launches).  -> that round's plan"""
    to_hand_over(P)
    P.plan(p(0.106))
    P.finish(0.07, tie=tie)
    out = P.plan(p(0.106))
    P.finish(0.07, tie=tie, far=far)
    return out


@pytest.fixture
def planner(lib):
    made = []

    def make(**kw):
        made.append(Planner(lib, **kw))
        return made[-1]
    yield make
    for P in made:
        P.close()


def test_first_search(planner):
    g, r, need = planner().plan(p(0.30))
    assert g == G()
    assert r == rows(E0_FIRST, A_FIRST)
    assert need == []


def test_auto_stays_tile_while_contracting_then_hands_over(planner):
    P = planner()
    plans = to_hand_over(P)
    # round 2: 0.2 is outside 1.5 x cell.  round 3: 0.09 is inside, but less than half of 0.2: still contracting
    for g, r, _ in plans[1:3]:
        assert g == G(same_active_set=1)
        assert r == rows(E0_KEPT, A_MOVED)
    # round 4: 0.08 > 0.5 x 0.09 and inside 1.5 x cell: the hand-over round is the tile kernel's bounds-leaving build
    g, r, _ = plans[3]
    assert g == G(same_active_set=1, tile_lb=1, handed_over=1)
    assert r == rows(E0_KEPT, A_MOVED)
    assert P.history()["auto_last_method"] == GRID and P.history()["nn_cache_valid"] == 1


def test_hand_over_without_tile_bounds_is_a_grid_round(planner):
    P = planner(tile_bounds=0)
    g, r, _ = to_hand_over(P)[3]
    assert g == G(same_active_set=1, method=GRID, far_launched=1)
    assert r == rows(E0_KEPT, A_MOVED)
    assert P.history()["auto_last_method"] == GRID


@pytest.mark.parametrize("step,ratio,eps,on_mfma", [(0.004, 3.0, 2.0, 0), (0.008, 3.0, 4.0, 1), (0.008, 0.0, -1.0, 0), (0.004, 1.5, 2.0, 1)])
def test_cache_aware_tile_round_picks_the_build_by_eps_over_mu(planner, step, ratio, eps, on_mfma):
    """mu = tile_mu x cell = 0.002; the queries of every edge moved by `step`, so the median eps / mu is step / 0.002"""
    P = planner(cache_mfma_ratio=ratio)
    to_hand_over(P)
    g, r, _ = P.plan(p(0.11 - step))
    assert g == G(same_active_set=1, tile_lb=1, tile_cached=1, handed_over=1, eps_over_mu=eps, cached_on_mfma=on_mfma)
    assert r == rows(E0_KEPT, A_CACHED)


@pytest.mark.parametrize("tie,far", [(0, 0), (3, 0), (0, 7), (2, 2)])
def test_bit_identical_poses_twice(planner, tie, far):
    P = planner()
    g, r, _ = to_fixed_point(P, tie=tie, far=far)
    # first round at the fixed point: tie_skip exactly when the last tie word was 0; last round was a tile round, so the far word is unknown
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=int(tie == 0),
                  tie_launched=int(tie != 0), far_launched=1, sel_skip=1)
    assert r == rows(E0_KEPT, A_SAME)
    # second: far_skip exactly when the last far word was 0 and that search ran the grid kernel; the medians of the last two rounds agree, so
    # the bracket is on
    g, r, _ = P.plan(p(0.106))
    m = 0.07 * 0.07
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=int(tie == 0),
                  tie_launched=int(tie != 0), far_skip=int(far == 0), far_launched=int(far != 0), sel_skip=1, use_bracket=1)
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006))


def test_select_is_skipped_with_a_queued_evaluation_only_if_the_last_select_wrote_the_scales(planner):
    P = planner()
    to_fixed_point(P)
    assert P.history()["sel_result_valid"] == 1 and P.history()["sel_result_armed"] == 0
    P.L.plan_solved(P.h, 1, 0, 1, 1)
    g, _, _ = P.plan(p(0.106))
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=1, tie_launched=0,
                  far_skip=1, sel_skip=0, use_bracket=1, spec_arm=1)
    assert P.finish(0.07) == 1                                   # armed slot 1, scales = (float)(1.5 sqrt(median)): the queued evaluation is usable
    assert P.history()["sel_result_armed"] == 1
    g, _, _ = P.plan(p(0.106))
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=1, tie_launched=0,
                  far_skip=1, sel_skip=1, use_bracket=1, spec_arm=1)
    P.option("sel_reuse", 0)
    assert P.plan(p(0.106))[0]["sel_skip"] == 0


def test_fixed_point_with_an_exchange_configured(planner):
    """(Where the select kernels put their results — the exchanged tail — is the executor's; here: the plan never skips the select or plans
    the second evaluation, and the arrival is read from exchanged data: armed = world, the scales of ALL edges.)"""
    P = planner(exchange=1, world=2, frame_flags=(7, 7, 7))
    to_fixed_point(P)
    P.L.plan_solved(P.h, 1, 0, 1, 1)
    P.L.plan_candidate(P.h, p(0.106).ctypes.data, 1, 1)
    g, r, _ = P.plan(p(0.106))
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=1, tie_launched=0,
                  far_skip=1, sel_skip=0, use_bracket=1, spec_arm=1, spec2_plan=0)
    assert P.finish(0.07, armed=1.0) == 0                        # one of two ranks armed: not usable
    assert P.history()["sel_result_valid"] == 0
    P.plan(p(0.106))
    assert P.finish(0.07, armed=2.0) == 1
    P.plan(p(0.106))
    assert P.finish(0.07, armed=2.0, redone=1) == 0              # the select was redone: the queued evaluation used the failed select's scales


def test_with_an_exchange_the_bracket_waits_for_the_peers_edges(planner):
    """Two ranks; this one owns edges 0 and 1, the peer edges 2 and 3.  The medians of all edges arrive exchanged.  This rank's edge 1 has
    settled, the peer's edge 3 has not: no bracket here either -- the decision a single process takes, which holds all four -- so that no
    rank arms a bracket that another rank's median then leaves.  Once edge 3 has settled the bracket is on, for the edges this rank owns."""
    P = planner(exchange=1, world=2, owned=(1, 1, 0, 0))
    P.plan(p(0.1)); P.finish(0.07)
    g, r, _ = P.plan(p(0.1))
    assert [row[0] for row in r] == [0, 1, 0, 0] and [row[1] for row in r] == [1, 0, 0, 0]      # (active: owned and searched; src_fixed)
    P.finish([0.07, 0.07, 0.07, 0.08])
    g, r, _ = P.plan(p(0.1))
    m = 0.07 * 0.07
    assert g["use_bracket"] == 0 and [row[7:] for row in r] == [(0.0, 0.0), (m * 0.994, m * 1.006), (0.0, 0.0), (0.0, 0.0)]
    P.finish([0.07, 0.07, 0.07, 0.08])
    g, r, _ = P.plan(p(0.1))
    assert g["use_bracket"] == 1 and [row[7:] for row in r] == [(0.0, 0.0), (m * 0.994, m * 1.006), (0.0, 0.0), (0.0, 0.0)]
    # and the same medians with every edge owned (a single process): the same two decisions
    Q = planner()
    Q.plan(p(0.1)); Q.finish(0.07)
    Q.plan(p(0.1)); Q.finish([0.07, 0.07, 0.07, 0.08])
    assert Q.plan(p(0.1))[0]["use_bracket"] == 0
    Q.finish([0.07, 0.07, 0.07, 0.08])
    assert Q.plan(p(0.1))[0]["use_bracket"] == 1


def test_cutoff_change(planner):
    P = planner()
    to_fixed_point(P)
    g, r, _ = P.plan(p(0.106), cutoff=0.02)
    # no cache for any edge (slot -1), no unchanged edge (every epoch bumps); AUTO still sees valid bounds and moving (not "same") edges: a
    # cache-aware tile round whose kernels find the cache switched off.  eps = 0: nothing moved
    m = 0.07 * 0.07
    assert g == G(same_active_set=1, tile_lb=1, tile_cached=1, handed_over=1, eps_over_mu=0.0, use_bracket=1)
    assert r == rows(E0_FIRST, A_MOVED[:6] + (m * 0.994, m * 1.006))


def test_fixed_mask_change(planner):
    P = planner()
    to_fixed_point(P)
    gone = (0, 1, 0, 0, 1, -1, 0.0, 0.0)                         # edge 3 (source: frame 2) is no longer searched: not unchanged, its list is dropped
    m = 0.07 * 0.07
    g, r, _ = P.plan(p(0.106), fixed=[1, 0, 1])
    assert g == G(method=GRID, all_same=1, same_active_set=0, far_narrow=1, far_launched=1, use_bracket=1)
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006), gone)
    P.finish(0.07)
    g, r, _ = P.plan(p(0.106), fixed=[1, 0, 1])                  # inactive then and now, empty: unchanged
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=1, tie_launched=0,
                  far_skip=1, sel_skip=1, use_bracket=1)
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006), (0, 1, 0, 1, 1, -1, 0.0, 0.0))
    P.finish(0.07)
    # newly active: no cache, a dirty list, no median: no bracket for the round.  Not every edge is "same" and the bounds are valid: AUTO runs
    # a cache-aware tile round (nothing moved: eps = 0)
    g, r, _ = P.plan(p(0.106), fixed=FIXED)
    assert g == G(same_active_set=0, tile_lb=1, tile_cached=1, handed_over=1, eps_over_mu=0.0)
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006), A_FIRST)


@pytest.mark.parametrize("how", ["forget", "tie_rule"])
def test_forget_makes_the_next_search_a_first_search(planner, how):
    P = planner()
    to_fixed_point(P)
    P.L.plan_solved(P.h, 1, 0, 1, 1)
    if how == "forget":                                            # mvicp_reset_history, a search that did not return OK
        P.L.plan_forget(P.h)
    else:                                                          # the rule is an input of the search: a flip forgets
        P.option("tie_rule", 0)
    g, r, need = P.plan(p(0.106))
    assert g == G(tie_launched=int(how == "forget"))
    assert r == rows(E0_FIRST, A_FIRST)
    assert need == []


def test_explicit_list_on_one_edge(planner):
    P = planner()
    to_fixed_point(P)
    P.L.plan_explicit(P.h, 2, 50, 0.1)                             # mvicp_set_correspondences(edge 2): also voids the temporal cache
    g, r, _ = P.plan(p(0.106))
    assert g == G(method=GRID, same_active_set=1, far_launched=1)
    kept = (1, 0, 0, 1, 0, -1, 0.07 * 0.07 * 0.994, 0.07 * 0.07 * 1.006)    # edges 1, 3: unchanged, list kept, medians settled
    assert r == [E0_KEPT, kept[:2] + (200,) + kept[2:], (1, 0, 200, 0, 0, 1, -1, 0.0, 0.0), kept[:2] + (300,) + kept[2:]]


def test_bracket_needs_every_active_edge_settled(planner):
    P = planner()
    to_hand_over(P)
    P.round(p(0.106), 0.07)
    P.round(p(0.106), [0.07, 0.07, 0.07, 0.07 * 1.001])            # edge 3's median d2 moves by 0.2 %
    g, r, _ = P.plan(p(0.106))
    assert g["use_bracket"] == 0 and g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=1,
                                            tie_launched=0, far_skip=1, sel_skip=1)
    m = 0.07 * 0.07
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006), A_SAME)
    P.finish([0.07, 0.07, 0.07, 0.07 * 1.001])
    g, r, _ = P.plan(p(0.106))                                     # now within 0.1 % on every active edge
    m3 = (0.07 * 1.001) * (0.07 * 1.001)
    assert g["use_bracket"] == 1
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006), A_SAME[:6] + (m3 * 0.994, m3 * 1.006))


@pytest.mark.parametrize("method", [GRID, TILE])
def test_forced_method_without_a_grid_is_brute(planner, method):
    g, r, _ = planner(frame_flags=(5, 5, 4)).plan(p(0.30), method=method)
    assert g == G(method=BRUTE)
    assert r == rows(E0_FIRST, A_FIRST)


def test_unknown_method_is_an_argument_error_from_the_planner(planner):
    g, _, _ = planner().plan(p(0.30), method=99)
    assert g == G(status=ERR_ARG, method=99)


def test_nn_cell_switches_by_the_predicted_distance_and_is_never_a_no_op(planner):
    P = planner(nn_cell=1)
    P.round(p(0.30), 0.12)
    g, r, _ = P.round(p(0.20), 0.09)                               # 0.12 is not below auto_switch x cell = 0.1
    assert g == G(same_active_set=1)
    g, r, _ = P.round(p(0.19), 0.09)                               # 0.09 is: the grid method, with no hand-over round
    assert g == G(same_active_set=1, method=GRID, far_launched=1)
    assert r == rows(E0_KEPT, A_MOVED)
    g, r, _ = P.round(p(0.19), 0.09)
    assert g == G(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, far_narrow=1, far_launched=1, use_bracket=1)
    m = 0.09 * 0.09
    assert r == rows(E0_KEPT, A_SAME[:6] + (m * 0.994, m * 1.006))


def test_spec_arm_needs_a_solve_and_sorted_normals_for_a_plane_objective(planner):
    # (the medians fed alternate between 0.2 and 0.21: outside 1.5 x cell, so every round is a tile round, and never settled, so no bracket)
    P = planner(frame_flags=(5, 5, 1))                             # frame 2 (target of edge 2, whose source is free) has no sorted normals
    assert P.round(p(0.30), 0.2)[0] == G()                         # no solve yet
    P.L.plan_solved(P.h, 1, 0, 1, 1)                               # a plane solve
    assert P.round(p(0.20), 0.21)[0] == G(same_active_set=1, spec_arm=0)
    P.L.plan_solved(P.h, 1, 0, 0, 1)                               # a point solve needs none
    assert P.round(p(0.19), 0.2)[0] == G(same_active_set=1, spec_arm=1)
    P.L.plan_solved(P.h, 0, 0, 0, 0)                               # a failed solve
    assert P.round(p(0.18), 0.21)[0] == G(same_active_set=1, spec_arm=0)
    P.L.plan_solved(P.h, 1, 0, 0, 1)
    P.option("spec_eval", 0)
    assert P.round(p(0.17), 0.2)[0] == G(same_active_set=1, spec_arm=0)
    P.option("spec_eval", 1)
    assert P.round(p(0.16), 0.21)[0] == G(same_active_set=1, spec_arm=1)


def test_spec2_plan_needs_identical_poses_the_same_edges_and_matching_flags(planner):
    fp = dict(method=GRID, all_same=1, same_active_set=1, all_unchanged=1, nothing_can_change=1, far_narrow=1, tie_skip=1, tie_launched=0, far_skip=1,
              use_bracket=1, spec_arm=1)
    P = planner()
    to_fixed_point(P)
    P.L.plan_solved(P.h, 1, 0, 1, 1)
    assert P.round(p(0.106), 0.07)[0] == G(spec2_plan=0, **fp)      # no candidate evaluation recorded
    P.L.plan_candidate(P.h, p(0.1).ctypes.data, 1, 1)
    assert P.round(p(0.106), 0.07)[0] == G(spec2_plan=1, sel_skip=1, **fp)
    P.L.plan_candidate(P.h, p(0.1).ctypes.data, 0, 1)              # the candidate was a point evaluation, the solve's flags say plane
    assert P.round(p(0.106), 0.07)[0] == G(spec2_plan=0, sel_skip=1, **fp)
    P.L.plan_candidate(P.h, p(0.1).ctypes.data, 1, 1)
    g, _, _ = P.round(p(0.106), 0.07, fixed=[1, 0, 1])              # another set of edges
    assert g == G(method=GRID, all_same=1, far_narrow=1, far_launched=1, spec_arm=1, use_bracket=1)
    g, _, _ = P.round(p(0.1061), 0.07, fixed=[1, 0, 1])             # poses that moved: a cache-aware round (eps / mu = 0.0001 / 0.002)
    assert g == G(same_active_set=1, tile_lb=1, tile_cached=1, handed_over=1, eps_over_mu=0.05, spec_arm=1, use_bracket=1)


def test_lazy_tie_trees(planner):
    assert planner().plan(p(0.30))[2] == []                                         # one rank, tie_lazy: no tree before a tie is reported
    assert planner(tie_lazy=0).plan(p(0.30))[2] == [0, 2, 1]                         # the targets of the active edges 1, 2, 3
    assert planner(exchange=1, world=2).plan(p(0.30))[2] == [0, 2, 1]
    assert planner(exchange=1, world=2, frame_flags=(5, 5, 7)).plan(p(0.30))[2] == [0, 1]
    assert planner(exchange=1, world=2, tie_rule=0).plan(p(0.30))[2] == []


def test_the_header_compiles_alone(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "search_plan.h"\n')
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], timeout=120)
    text = open(os.path.join(CSRC, "search_plan.h")).read()
    assert "#include <hip" not in text and '#include "common.h"' not in text


def test_the_replay_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/plan_replay_main.cpp: a program of its own that replays the transitions above (first search ... forget) through the harness
    functions, built with -fsanitize=address,undefined and run as a plain executable"""
    exe = str(tmp_path / "plan_replay")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "plan_replay_main.cpp")], timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    txt = out.stdout.decode()
    assert out.returncode == 0 and "PLAN_REPLAY_OK" in txt, txt[-4000:]
    assert "runtime error" not in txt and "AddressSanitizer" not in txt, txt[-4000:]
