"""-m gpu: reject masks where tests/test_gpu_reject_mask.py does not go.  The reference is that file's: a second, MASKLESS engine run through the
same calls at the same poses, method and options, followed by tests/rejectref.py (maskcases.expected_lists); every comparison is byte for byte.

  a. the in-place upkeep (update_list_entry, csrc/nn_list.h) under a mask with every method FORCED: moving rounds on valid lists through
     nn_grid_kernel / nn_cell_kernel / nn_far_kernel / the tie kernels, the tile and the mfma builds and the brute-force kernel, with mask
     changes at moved poses;
  b. the random scripts of tests/regime_seq.py (method and option flips, resets, failed searches, tie-rule flips) with masks on from round 0
     and mask changes after a "hold", between two solves (a queued evaluation is armed) and to all-ones;
  c. a mask change that throws an edge's median out of the bracket of the one-pass select;
  d. a solve between a mask change and the next search, with the queued evaluation on and off;
  e. exact ties: duplicated targets of which exactly one copy is flagged, under both tie rules (the tie kernels rewrite the neighbour and run
     the upkeep a second time, with an acceptance that may flip between the two calls)."""
import numpy as np
import pytest

import maskcases
import mvicp
import regime_seq
import test_reject_mask_cases_cpu as cases
from maskcases import S, T
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu

K, N = 4, 3000        # a source of 3 000 points: three compaction blocks, the last one partial, and twelve dirty slots
CUTOFF = 0.05
SE3 = L.PARAM_SOPHUS_SE3


def engines(pts, nor, src, dst, options=()):
    out = []
    for _ in range(2):
        e = mvicp.Engine(0)
        for name, value in options:
            e.set_option(name, value)
        e.set_frames(pts, nor); e.set_graph(src, dst)
        out.append(e)
    return out


@pytest.fixture(scope="module")
def pb():
    return synth.make_problem(K, N)


def _ev(kind, **kw):
    return dict(kind=kind, param=2, plane=1, robust=True, **kw)


# ---------------------------------------------------------------- a. forced methods on valid lists
CONFIGS = {
    # (nn_cell_kernel needs the brick map, which exists for the cell-curve orders only: grid_curve 1, set before the upload)
    "grid-cell": (L.NN_GRID, (("grid_curve", 1), ("nn_cell", 1)), "grid"),
    "grid": (L.NN_GRID, (("nn_cell", 0),), "grid"),
    "tile": (L.NN_TILE, (("tile_mfma", 0),), "tile<"),
    "mfma": (L.NN_TILE, (("tile_mfma", 2),), "mfma<"),
    "brute": (L.NN_BRUTE, (), "brute"),
}


def forced_script(pb, method):
    """a first search, five moving rounds, identical poses twice, a new mask on frame 2 and a moving round, frame 1's mask cleared, a cutoff
    change, the halfspace mask on frame 0 as TARGET, two moving rounds, identical poses"""
    return ([_ev("method", method=method)] + [_ev("none")] * 5 + [_ev("hold"), _ev("hold"),
            _ev("mask", frame=2, mask=maskcases.random_mask(N, 0.1, 700), roles=T | S, tag="new"), _ev("none"),
            _ev("mask", frame=1, mask=None, roles=0, tag="clear"), _ev("cutoff", cutoff=0.02),
            _ev("mask", frame=0, mask=maskcases.halfspace_mask(pb["pts"][0], 1, 0.7), roles=T, tag="halfspace"),
            _ev("none"), _ev("none"), _ev("hold")])


@pytest.mark.parametrize("config", list(CONFIGS))
def test_forced_method_rounds_keep_masked_lists_in_place(pb, config):
    """After every search: lists, counts and weights = maskless + rejectref; the same launch on both engines; the same census (a mask costs no
    cache hit).  For the grid configurations the far kernel must have run, on queries of its own, in a masked moving round on valid lists."""
    method, options, launch = CONFIGS[config]
    eng, ref = engines(pb["pts"], pb["nor"], pb["src"], pb["dst"], options)
    E = len(pb["src"])
    masks = maskcases.standard_masks([N] * K)
    scopes = ["nn_far", "nn_tie"]
    last = {"key": None, "epochs": None, "scopes": {s: 0 for s in scopes}}
    seen = {"launches": set(), "identical": 0, "far_rounds": 0, "hits": 0.0}
    try:
        for f, (m, r) in masks.items():
            eng.set_reject_mask(f, m, r)
        for e_ in (eng, ref):
            e_.profile(True); e_.profile_reset(); e_.set_option("nn_census", 1)
        last["eng"], last["ref"] = eng.nn_census(), ref.nn_census()

        def extra(st, rc):
            rnd, ev = st["round"], st["event"]
            nn = eng.last_nn_launch()
            assert nn == ref.last_nn_launch(), (rnd, nn, ref.last_nn_launch())
            assert nn.startswith(launch), (config, rnd, nn)
            seen["launches"].add(nn)
            ce, cr = eng.nn_census(), ref.nn_census()
            de = {k: ce[k] - last["eng"][k] for k in ce}; dr = {k: cr[k] - last["ref"][k] for k in cr}
            now = {s: int(eng.profile_get(s)[1]) for s in scopes}
            ds = {s: now[s] - last["scopes"][s] for s in scopes}
            print("%-9s round %2d %-6s %-9s %-22s nn_far %d nn_tie %d launches | far %5.0f hits %6.0f of %6.0f queries | kept %d of %d" % (
                config, rnd, ev["kind"], ev.get("tag", ""), nn, ds["nn_far"], ds["nn_tie"], de["far"], de["hits"], de["queries"], int(st["counts"].sum()), int(rc.sum())))
            if config == "grid-cell":
                # nn_cell_kernel's four waves draw their LDS staging space from one pool per workgroup (s_pool, an atomic): which wave runs
                # out of it, and sends its lanes to the far list, depends on the order the waves arrive in.  Its "far", "nodes", "candidates"
                # and "fetched" figures differ between two runs of the same search on two maskless engines, and so may the next round's "hits":
                # the far path leaves another (equally valid) lower bound for the temporal cache than the staged path.
                assert de["queries"] == dr["queries"], (rnd, nn, de, dr)
            else:
                assert de == dr, (rnd, nn, de, dr)
            assert 0 < int(st["counts"].sum()) < int(rc.sum())
            # a masked moving round on lists that the search before left valid
            if method == L.NN_GRID and rnd >= 1 and ev["kind"] == "none" and ds["nn_far"] > 0 and de["far"] > 0:
                seen["far_rounds"] += 1
            seen["hits"] += dr["hits"]
            # which grid kernel ran: the per-lane kernel fetches every candidate it examines, the cell-staging kernel stages points into LDS
            # once per wave and scans them from there (the census of api.cpp)
            seen["staged"] = seen.get("staged", False) or de["fetched"] != de["candidates"]
            key = (st["poses"].tobytes(), st["fixed"].tobytes(), st["cutoff"], st["method"])
            epochs = eng.correspondence_epochs()
            if key == last["key"] and ev["kind"] != "mask":          # identical inputs: every epoch stays
                assert epochs.tobytes() == last["epochs"].tobytes(), (rnd, epochs, last["epochs"])
                seen["identical"] += 1
            last.update(eng=ce, ref=cr, scopes=now, key=key, epochs=epochs)

        log = regime_seq.run(eng, pb, forced_script(pb, method), after_search=maskcases.anchor_hook(eng, ref, pb, seen, extra), masks=masks)
    finally:
        eng.close(); ref.close()
    print(config, "launched", sorted(seen["launches"]))
    assert seen["searches"] == 16 and seen["identical"] >= 1, seen
    assert not np.array_equal(log[-1][2], pb["init"])
    if method == L.NN_GRID:
        assert seen["far_rounds"] >= 1, seen
        assert seen["staged"] == (config == "grid-cell"), seen


# ---------------------------------------------------------------- a'. a neighbour that becomes flagged, on a list that is kept in place
STEP = 3e-3


@pytest.mark.parametrize("config", ["grid-cell", "grid", "tile", "mfma", "auto"])
def test_a_new_neighbour_that_is_flagged_drops_the_pair_in_place(pb, config):
    """The one case in which the masks of ListRef decide the ANSWER and not only whether an edge is rebuilt.  With a mask pointer missing, a
    query that only the mask keeps out of the list looks accepted, its edge is declared dirty and the compaction -- which has the masks from
    its own table -- rebuilds the list correctly: slower, never wrong.  Here no such query exists when the lists are built: the mask of a
    target flags exactly the points that are nobody's neighbour at the poses A and somebody's at the poses B (A: the ground truth, B: 3 mm
    away; from the maskless lists alone).  At A the masked search drops nothing; from A to B no query changes its acceptance by the cutoff
    (the maskless lists hold the same sources), so every list is kept in place, and the queries whose NEW neighbour is flagged must leave it
    through update_list_entry's own reading of the target's mask."""
    method, options, _ = CONFIGS[config] if config != "auto" else (L.NN_AUTO, (), "")
    eng, ref = engines(pb["pts"], pb["nor"], pb["src"], pb["dst"], options)
    E, fx = len(pb["src"]), pb["fixed"]
    A = pb["gt"].copy(); B = A.copy()
    for k in range(1, K):
        B[k][:3, 3] += STEP * np.array([1.0, -0.5, 0.25]) * (1.0 if k % 2 else -1.0)
    try:
        ref.correspond(A, fx, CUTOFF, method); ref.correspond(A, fx, CUTOFF, method)
        la = maskcases.lists(ref, E)
        ref.correspond(B, fx, CUTOFF, method)
        lb = maskcases.lists(ref, E)
        masks = {}
        for d in range(K):
            m = np.zeros(N, dtype=np.uint8)
            for e in range(E):
                if pb["dst"][e] == d:
                    m[lb[e][1]] = 1
            for e in range(E):
                if pb["dst"][e] == d:
                    m[la[e][1]] = 0
            masks[d] = (m, T)
        want_a, want_b = maskcases.expected_lists(pb, la, masks), maskcases.expected_lists(pb, lb, masks)
        # input conditions, from the maskless lists alone
        assert all(want_a[e][0].tobytes() == la[e][0].tobytes() for e in range(E))                   # at A the masks drop nothing
        assert all(la[e][0].tobytes() == lb[e][0].tobytes() for e in range(E))                       # A -> B: no acceptance changes by the cutoff
        dropped = [len(lb[e][0]) - len(want_b[e][0]) for e in range(E)]
        print(config, "pairs whose new neighbour is flagged, per edge:", dropped)
        assert sum(1 for n in dropped if n >= 100) >= 4, dropped
        for d, (m, r) in masks.items():
            eng.set_reject_mask(d, m, r)
        for tag in ("A", "A again"):
            c, w = eng.correspond(A, fx, CUTOFF, method)
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, want_a, (config, tag))
        c, w = eng.correspond(B, fx, CUTOFF, method)
        maskcases.assert_lists(maskcases.lists(eng, E), c, w, want_b, (config, "B"))
        assert eng.last_nn_launch() == ref.last_nn_launch()
        c, w = eng.correspond(A, fx, CUTOFF, method)                                                # and back: the dropped pairs return
        maskcases.assert_lists(maskcases.lists(eng, E), c, w, want_a, (config, "back at A"))
    finally:
        eng.close(); ref.close()


# ---------------------------------------------------------------- b. random scripts under masks
@pytest.mark.parametrize("seed,extended", cases.PATH_SCRIPTS)
def test_random_scripts_under_masks(pb, seed, extended):
    """(Seed 2 beside the seeds 0, 1, 100: it is the one whose script forces a method.)"""
    base = regime_seq.script(seed, K, extended=extended)
    events = maskcases.with_mask_events(base, maskcases.standard_schedule(base, [N] * K))
    kinds = [e["kind"] for e in base]
    assert "reset" in kinds and (seed != 100 or ("fail" in kinds and "tie_rule" in kinds)) and (seed != 2 or "method" in kinds) and (seed != 0 or "option" in kinds), kinds
    eng, ref = engines(pb["pts"], pb["nor"], pb["src"], pb["dst"])
    E = len(pb["src"])
    masks = maskcases.standard_masks([N] * K)
    into1 = np.array([pb["dst"][e] == 1 for e in range(E)])
    seen = {"ones_rounds": 0}
    try:
        for f, (m, r) in masks.items():
            eng.set_reject_mask(f, m, r)

        def extra(st, rc):
            m1, r1 = st["masks"][1]
            if m1 is not None and m1.all() and r1 == T:
                assert not st["counts"][into1].any() and not st["weights"][into1].any(), (st["round"], st["counts"], st["weights"])
                seen["ones_rounds"] += 1
            print("seed %3d round %2d %-8s %-12s %-22s kept %6d of %6d" % (seed, st["round"], st["event"]["kind"], st["event"].get("tag", ""), eng.last_nn_launch(),
                                                                        int(st["counts"].sum()), int(rc.sum())))

        def after_round(st):
            assert np.isfinite(st["poses"]).all(), st["round"]

        log = regime_seq.run(eng, pb, events, after_search=maskcases.anchor_hook(eng, ref, pb, seen, extra), after_round=after_round, masks=masks)
    finally:
        eng.close(); ref.close()
    assert seen["searches"] == len(events) and seen["ones_rounds"] >= 2, seen
    assert not np.array_equal(log[-1][2], pb["init"])


# ---------------------------------------------------------------- c. the bracket of the one-pass select
def test_a_mask_change_that_leaves_the_select_bracket(pb):
    E = len(pb["src"])
    P, fx = pb["init"], pb["fixed"]
    before = maskcases.standard_masks([N] * K)
    f = cases.BRACKET["frame"]
    after = dict(before)
    after[f] = (maskcases.halfspace_mask(pb["pts"][f], cases.BRACKET["axis"], cases.BRACKET["quantile"]), S)
    got = {}
    for bracket in (1, 0):
        eng, ref = engines(pb["pts"], pb["nor"], pb["src"], pb["dst"], (("sel_bracket", bracket),))
        try:
            for k, (m, r) in before.items():
                eng.set_reject_mask(k, m, r)
            for _ in range(3):                                   # a first search and two more at the same poses: every median has settled
                c, w = eng.correspond(P, fx, CUTOFF)
                ref.correspond(P, fx, CUTOFF)
            ref_lists = maskcases.lists(ref, E)
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, maskcases.expected_lists(pb, ref_lists, before), ("settled", bracket))
            shift = cases.median_shift(pb, ref_lists, before, after)
            print("sel_bracket %d: relative change of the median d2 per edge under the new mask:" % bracket, ["%.4f" % s for s in shift])
            assert max(shift[e] for e in range(E) if pb["src"][e] == f) > 0.006, shift       # input condition, from the maskless lists alone
            eng.set_reject_mask(f, *after[f])
            c, w = eng.correspond(P, fx, CUTOFF)
            ref.correspond(P, fx, CUTOFF)
            got[bracket] = (c.tobytes(), w.tobytes(), [tuple(a.tobytes() for a in l) for l in maskcases.lists(eng, E)])
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, maskcases.expected_lists(pb, maskcases.lists(ref, E), after), ("out of the bracket", bracket))
            c, w = eng.correspond(P, fx, CUTOFF)                 # and the search after it, with the medians of the new mask
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, maskcases.expected_lists(pb, maskcases.lists(ref, E), after), ("again", bracket))
        finally:
            eng.close(); ref.close()
    assert got[1] == got[0]


# ---------------------------------------------------------------- d. a solve between a mask change and the next search
def test_a_solve_between_a_mask_change_and_the_next_search(pb):
    """search, solve, search (its first evaluation is queued), MASK CHANGE, solve, search, solve.  Until the next search the lists on the device
    are the last search's (include/mvicp.h): the solve after the change runs over them, and they read back unchanged."""
    E = len(pb["src"])
    fx = pb["fixed"]
    before = maskcases.standard_masks([N] * K)
    after = dict(before)
    after[2] = (maskcases.halfspace_mask(pb["pts"][2], 2, 0.6), T | S)
    poses = {}
    for spec in (1, 0):
        eng, ref = engines(pb["pts"], pb["nor"], pb["src"], pb["dst"], (("spec_eval", spec),))
        try:
            eng.profile(True)
            for k, (m, r) in before.items():
                eng.set_reject_mask(k, m, r)
            P = pb["init"].copy()
            eng.correspond(P, fx, CUTOFF)
            P, _ = eng.optimize(P, fx, SE3, True, True, 50)
            c, w = eng.correspond(P, fx, CUTOFF)
            ref.correspond(P, fx, CUTOFF)
            want = maskcases.expected_lists(pb, maskcases.lists(ref, E), before)
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, want, ("before the change", spec))
            eng.set_reject_mask(2, *after[2])
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, want, ("after the change", spec))
            P, _ = eng.optimize(P, fx, SE3, True, True, 50)
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, want, ("after the solve", spec))
            c, w = eng.correspond(P, fx, CUTOFF)
            ref.correspond(P, fx, CUTOFF)
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, maskcases.expected_lists(pb, maskcases.lists(ref, E), after), ("the next search", spec))
            P, _ = eng.optimize(P, fx, SE3, True, True, 50)
            hits = eng.profile_get("spec.hit")[1]
            print("spec_eval %d: %d evaluations served from the queue" % (spec, hits))
            assert (hits > 0) == bool(spec)
            poses[spec] = P
        finally:
            eng.close(); ref.close()
    assert poses[1].tobytes() == poses[0].tobytes() and not np.array_equal(poses[1], pb["init"])


# ---------------------------------------------------------------- e. exact ties
METHODS = {"grid": L.NN_GRID, "tile": L.NN_TILE, "auto": L.NN_AUTO, "brute": L.NN_BRUTE}
N0 = 3000


@pytest.fixture(scope="module")
def tie_world():
    """3 x 4 000 points, a third of them twice; per frame, as TARGET, one point of every duplicated pair is flagged.  Input condition, from
    maskless engines alone (rule 1 and rule 0, brute force, the ground-truth poses): queries whose neighbour differs between the rules with
    exactly one of the two picks flagged exist in both directions, and every edge's masked list differs between the rules in `first`."""
    pb3 = synth.make_problem(3, N0)
    pts, nor, picks = maskcases.dup_clouds(pb3)
    world = {"pb": pb3, "pts": pts, "nor": nor, "E": len(pb3["src"])}
    for swap in (False, True):
        world[swap] = {k: (maskcases.duplicate_pair_mask(N0, picks[k], swap), T) for k in range(3)}
    ref_lists = {}
    for rule in (0, 1):
        B = mvicp.Engine(0)
        try:
            B.set_option("tie_rule", rule)
            B.set_frames(pts, nor); B.set_graph(pb3["src"], pb3["dst"])
            B.correspond(pb3["gt"], pb3["fixed"], CUTOFF, L.NN_BRUTE)
            ref_lists[rule] = maskcases.lists(B, world["E"])
        finally:
            B.close()
    only0 = only1 = 0
    want = {rule: maskcases.expected_lists(pb3, ref_lists[rule], world[False]) for rule in (0, 1)}
    for e in range(world["E"]):
        (f0, s0, d0), (f1, s1, d1) = ref_lists[0][e], ref_lists[1][e]
        assert f0.tobytes() == f1.tobytes() and d0.tobytes() == d1.tobytes(), e
        m = world[False][int(pb3["dst"][e])][0]
        differ, a, b = s0 != s1, m[s0] != 0, m[s1] != 0
        only0 += int((differ & a & ~b).sum()); only1 += int((differ & ~a & b).sum())
    world["differ"] = [e for e in range(world["E"]) if want[0][e][0].tobytes() != want[1][e][0].tobytes()]
    print("queries whose picks differ with only rule 0's flagged: %d, only rule 1's: %d; masked lists differ in `first` on edges %s" % (only0, only1, world["differ"]))
    assert only0 > 0 and only1 > 0 and world["differ"] == list(range(world["E"])), (only0, only1, world["differ"])
    return world


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("method", list(METHODS))
def test_exact_ties_with_one_copy_flagged(tie_world, method, lazy):
    W = tie_world
    pb3, E, m = W["pb"], W["E"], METHODS[method]
    fx = pb3["fixed"]
    eng, ref = engines(W["pts"], W["nor"], pb3["src"], pb3["dst"], (("tie_lazy", lazy),))
    state = {"masks": W[False]}
    try:
        for k, (mask, r) in W[False].items():
            eng.set_reject_mask(k, mask, r)

        def search(P, tag):
            c, w = eng.correspond(P, fx, CUTOFF, m)
            rc, _ = ref.correspond(P, fx, CUTOFF, m)
            maskcases.assert_lists(maskcases.lists(eng, E), c, w, maskcases.expected_lists(pb3, maskcases.lists(ref, E), state["masks"]), (method, lazy, tag))
            assert 0 < int(c.sum()) < int(rc.sum())
            return eng.correspondence_epochs()

        def rule(value):
            eng.set_option("tie_rule", value); ref.set_option("tie_rule", value)

        P0 = pb3["gt"].copy()
        ep0 = search(P0, "first")
        assert np.array_equal(search(P0, "identical poses"), ep0)
        rule(0)
        ep1 = search(P0, "rule 0")
        assert sorted(np.nonzero(ep1 != ep0)[0].tolist()) == W["differ"], (ep0, ep1)      # the epochs change on the edges whose masked lists differ
        assert np.array_equal(search(P0, "rule 0 again"), ep1)
        rule(1)
        ep2 = search(P0, "rule 1 again")
        assert sorted(np.nonzero(ep2 != ep1)[0].tolist()) == W["differ"] and all(ep2[e] != ep0[e] for e in W["differ"]), (ep0, ep1, ep2)
        P = pb3["init"].copy()
        for r in range(4):
            search(P, "moving round %d" % r)
            P, _ = eng.optimize(P, fx, SE3, True, True, 50)
        state["masks"] = W[True]                                  # the other copy of every pair, at moved poses
        for k, (mask, r) in W[True].items():
            eng.set_reject_mask(k, mask, r)
        for r in range(3):
            search(P, "swapped, moving round %d" % r)
            P, _ = eng.optimize(P, fx, SE3, True, True, 50)
        assert np.isfinite(P).all() and not np.array_equal(P, pb3["init"])
    finally:
        eng.close(); ref.close()
