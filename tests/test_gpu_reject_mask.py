"""-m gpu: reject masks inside the search (mvicp_set_reject_mask, mvicp_boundary_adopt, mvicp_get_reject_mask).  The reference in every case is a
second, MASKLESS engine run through the same calls, followed by tests/rejectref.py: counts, lists, stored distances and weights equal it byte
for byte -- after one search with every method and role, after every search of a scripted registration that crosses the regimes of
mvicp_correspond (where the temporal cache must hit as often as on the maskless engine: the point of keeping the lists searched lists), and
across mask changes at unchanged poses; the evaluations over a masked search equal those over the kept lists installed on another engine; and
the registration of the partial pair ends where tests/test_reject_mask_cpu.py says."""
import numpy as np
import pytest

import maskcases
import matchref
import mvicp
import regime_seq
import rejectref
import search_trace
import symref
import test_reject_mask_cpu as cpu
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu

T, S = L.REJECT_AS_TARGET, L.REJECT_AS_SOURCE
K, N = 4, 3000        # a source of 3 000 points: three compaction blocks, the last one partial, and twelve dirty slots
CUTOFF = 0.05


@pytest.fixture(scope="module")
def world():
    pb = synth.make_problem(K, N)
    ref, eng = mvicp.Engine(0), mvicp.Engine(0)
    ref.set_frames(pb["pts"], pb["nor"]); eng.set_frames(pb["pts"], pb["nor"])
    rng = np.random.default_rng(20260)
    flags = [eng.boundary(i, 30)["flag"] for i in range(K)]
    # the boundary flags plus about 10 % at random: flagged points sit everywhere, not only on the rim
    masks = [np.ascontiguousarray(flags[i] | (rng.random(N) < 0.1), dtype=np.uint8) for i in range(K)]
    for i in range(K):
        assert 0 < int(flags[i].sum()) < N and int(flags[i].sum()) < int(masks[i].sum()) < N // 2
    ref.set_graph(pb["src"], pb["dst"]); eng.set_graph(pb["src"], pb["dst"])
    yield {"pb": pb, "ref": ref, "eng": eng, "flags": flags, "masks": masks, "E": len(pb["src"])}
    ref.close(); eng.close()


def set_all(eng, masks, roles):
    for i in range(K):
        eng.set_reject_mask(i, None if masks is None else masks[i], roles)


def lists(eng, E):
    return [eng.get_correspondences(e) for e in range(E)]


def expected(pb, ref_lists, masks, roles):
    """rejectref over the maskless engine's lists: `masks` per frame (an entry may be None), in `roles` -> per edge (first, second, dist, weight)"""
    return maskcases.expected_lists(pb, ref_lists, [(m, roles if m is not None else 0) for m in masks])


def assert_equals(got_lists, counts, weights, want, tag):
    for e, ((gf, gs, gd), (wf, ws, wd, ww)) in enumerate(zip(got_lists, want)):
        assert counts[e] == len(wf), (tag, e, int(counts[e]), len(wf))
        assert gf.tobytes() == wf.tobytes() and gs.tobytes() == ws.tobytes() and gd.tobytes() == wd.tobytes(), (tag, e)
        assert np.float32(weights[e]).tobytes() == np.float32(ww).tobytes(), (tag, e, weights[e], ww)


@pytest.fixture(scope="module")
def unmasked(world):
    """the maskless engine's first search at the initial poses, per method (computed once, never changed)"""
    pb, ref = world["pb"], world["ref"]
    out = {}
    for method in (L.NN_BRUTE, L.NN_GRID, L.NN_TILE, L.NN_AUTO):
        ref.reset_history()
        c, w = ref.correspond(pb["init"], pb["fixed"], CUTOFF, method)
        out[method] = (c, w, lists(ref, world["E"]))
    return out


@pytest.mark.parametrize("roles", [T, S, T | S])
@pytest.mark.parametrize("method", [L.NN_BRUTE, L.NN_GRID, L.NN_TILE, L.NN_AUTO])
def test_one_search_equals_the_reference_with_every_method_and_role(world, unmasked, method, roles):
    pb, eng, masks, E = world["pb"], world["eng"], world["masks"], world["E"]
    set_all(eng, masks, roles)
    try:
        eng.reset_history()
        counts, weights = eng.correspond(pb["init"], pb["fixed"], CUTOFF, method)
        got = lists(eng, E)
        c0, _, l0 = unmasked[method]
        assert_equals(got, counts, weights, expected(pb, l0, masks, roles), (method, roles))
        assert 0 < int(c0.sum()) - int(counts.sum()) < int(c0.sum())      # pairs were dropped, and pairs stayed
        triples, off = eng.map_correspondences()
        for e in range(E):
            t = triples[off[e]:off[e + 1]]
            assert t["first"].tobytes() == got[e][0].tobytes() and t["second"].tobytes() == got[e][1].tobytes() and t["dist"].tobytes() == got[e][2].tobytes()
    finally:
        set_all(eng, None, 0)


def _ev(kind, **kw):
    return dict(kind=kind, param=2, plane=1, robust=True, **kw)


# a first search, moving rounds up to and past the hand-over, bit-identical poses twice, a cutoff change, a fixed-mask change
SCRIPT = ([_ev("none")] * 9 + [_ev("hold"), _ev("hold"), _ev("none"), _ev("cutoff", cutoff=0.02), _ev("none"), _ev("hold"), _ev("none"),
          _ev("fixed", frame=2), _ev("none"), _ev("hold"), _ev("none"), _ev("fixed", frame=2), _ev("none"), _ev("hold"), _ev("none")])


def test_the_upkeep_paths_keep_the_lists_and_the_temporal_cache(world):
    """The masked engine solves; the maskless one searches at the same poses.  After every search: lists and weights = maskless + rejectref,
    byte for byte; the same kernel ran on both; and the census (queries, cache hits, ...) of the two launches is the same -- a build that
    routed rejection through explicit lists would have no temporal cache to hit (mvicp_set_correspondences invalidates it)."""
    pb, ref, eng, masks, E = world["pb"], world["ref"], world["eng"], world["masks"], world["E"]
    roles = T | S
    set_all(eng, masks, roles)
    seen = {"regimes": set(), "hits": 0.0, "identical": 0}
    last = {"eng": None, "ref": None, "mark": 0, "epochs": None, "key": None}
    try:
        for e_ in (eng, ref):
            e_.reset_history(); e_.profile(True); e_.profile_reset(); e_.set_option("nn_census", 1)
        last["eng"], last["ref"] = eng.nn_census(), ref.nn_census()
        last["mark"] = int(eng.profile_get(search_trace.MARK)[1])

        def after_search(st):
            rnd, kind = st["round"], st["event"]["kind"]
            rc, rw = ref.correspond(st["poses"], st["fixed"], st["cutoff"], st["method"])
            assert_equals(lists(eng, E), st["counts"], st["weights"], expected(pb, lists(ref, E), masks, roles), ("round", rnd, kind))
            assert 0 < int(st["counts"].sum()) < int(rc.sum())
            # the same launch, the same census
            nn = eng.last_nn_launch()
            assert nn == ref.last_nn_launch(), (rnd, nn, ref.last_nn_launch())
            ce, cr = eng.nn_census(), ref.nn_census()
            de = {k: ce[k] - last["eng"][k] for k in ce}; dr = {k: cr[k] - last["ref"][k] for k in cr}
            mark = int(eng.profile_get(search_trace.MARK)[1])
            bnd = search_trace.bounds_build(nn)
            regime = "tile" if bnd == 0 else ("cache-aware tile" if mark > last["mark"] else "hand-over") if bnd == 1 else nn
            print("round %2d %-6s %-28s %-16s masked hits %8.0f of %8.0f queries | maskless %8.0f of %8.0f | kept %d of %d" % (
                rnd, kind, nn, regime, de["hits"], de["queries"], dr["hits"], dr["queries"], int(st["counts"].sum()), int(rc.sum())))
            assert de == dr, (rnd, nn, de, dr)
            seen["regimes"].add(regime)
            if regime in ("cache-aware tile", "grid"):
                seen["hits"] += de["hits"]
            # bit-identical rounds: the same poses, fixed mask, cutoff and method as the search before -> every epoch stays
            key = (st["poses"].tobytes(), st["fixed"].tobytes(), st["cutoff"], st["method"])
            epochs = eng.correspondence_epochs()
            if key == last["key"]:
                assert epochs.tobytes() == last["epochs"].tobytes(), (rnd, epochs, last["epochs"])
                seen["identical"] += 1
            last.update(eng=ce, ref=cr, mark=mark, epochs=epochs, key=key)

        regime_seq.run(eng, pb, SCRIPT, after_search=after_search)
    finally:
        for e_ in (eng, ref):
            e_.set_option("nn_census", 0); e_.profile(False)
        set_all(eng, None, 0)
    # the script went where it was written to go, and the cache was hit there
    assert {"tile", "hand-over", "cache-aware tile", "grid"} <= seen["regimes"], seen["regimes"]
    assert seen["identical"] >= 2 and seen["hits"] > 0, seen


def test_mask_changes_between_searches_at_unchanged_poses(world, unmasked):
    pb, eng, masks, E = world["pb"], world["eng"], world["masks"], world["E"]
    P, fx = pb["init"], pb["fixed"]
    into1 = np.array([pb["dst"][e] == 1 for e in range(E)])
    assert into1.any() and not into1.all()
    c0, w0, l0 = unmasked[L.NN_AUTO]
    none = [None] * K
    try:
        eng.reset_history()
        eng.correspond(P, fx, CUTOFF)
        counts, weights = eng.correspond(P, fx, CUTOFF)
        ep0 = eng.correspondence_epochs()
        assert counts.tobytes() == c0.tobytes() and weights.tobytes() == w0.tobytes()

        def step(mask, roles, want_masks, tag):
            before = eng.correspondence_epochs()
            eng.set_reject_mask(1, mask, roles)
            assert eng.correspondence_epochs().tobytes() == before.tobytes()      # (the new epoch comes with the search that rebuilds the list)
            c, w = eng.correspond(P, fx, CUTOFF)
            after = eng.correspondence_epochs()
            assert_equals(lists(eng, E), c, w, expected(pb, l0, want_masks, T), tag)
            return c, w, (after != before)

        m1 = list(none); m1[1] = masks[1]
        c, w, changed = step(masks[1], T, m1, "set")
        assert changed.tolist() == into1.tolist() and int(c[into1].sum()) < int(c0[into1].sum())
        ep = eng.correspondence_epochs()
        c2, w2 = eng.correspond(P, fx, CUTOFF)                                    # nothing changed since: the same answer, and no epoch changes
        assert c2.tobytes() == c.tobytes() and w2.tobytes() == w.tobytes() and eng.correspondence_epochs().tobytes() == ep.tobytes()
        c, w, changed = step(None, T, none, "clear")
        assert changed.tolist() == into1.tolist() and c.tobytes() == c0.tobytes() and w.tobytes() == w0.tobytes()
        ones = list(none); ones[1] = np.ones(N, dtype=np.uint8)
        c, w, changed = step(ones[1], T, ones, "all ones")
        assert changed.tolist() == into1.tolist() and not c[into1].any() and not w[into1].any() and c[~into1].tobytes() == c0[~into1].tobytes()
        for plane in (False, True):   # an evaluation over empty lists is still well defined: their blocks are zero, the others are not
            blk = eng.linearize(P, plane, True)
            assert np.isfinite(blk).all() and not blk[into1].any() and np.abs(blk[~into1]).sum() > 0
        P2, sm = eng.optimize(P, fx, L.PARAM_SOPHUS_SE3, True, True, 50)
        assert np.isfinite(P2).all()
        zeros = list(none); zeros[1] = np.zeros(N, dtype=np.uint8)
        c, w, changed = step(zeros[1], T, zeros, "all zeros")
        assert changed.tolist() == into1.tolist() and c.tobytes() == c0.tobytes() and w.tobytes() == w0.tobytes()
        # a source-side mask bears on the edges OUT of the frame, and only on them
        out1 = np.array([pb["src"][e] == 1 for e in range(E)])
        assert out1.any() and not fx[1]
        eng.set_reject_mask(1, None)
        eng.correspond(P, fx, CUTOFF)
        before = eng.correspondence_epochs()
        eng.set_reject_mask(1, masks[1], S)
        c, w = eng.correspond(P, fx, CUTOFF)
        assert (eng.correspondence_epochs() != before).tolist() == out1.tolist()
        assert_equals(lists(eng, E), c, w, expected(pb, l0, m1, S), "source")
    finally:
        set_all(eng, None, 0)


def _blocks(eng, P):
    return {"point": eng.linearize(P, False, True), "plane": eng.linearize(P, True, True),
            "symmetric": eng.linearize_metric(P, L.METRIC_SYMMETRIC, True), "gicp": eng.linearize_gicp(P, 1e-3, True)}


def test_evaluations_over_a_masked_search(world, unmasked):
    """Compared with an engine that holds the kept lists as explicit lists at the reference weights.  Control first: the same comparison
    without a mask.  Where the control is byte-equal, so must the masked comparison be; where it is not, the two paths sum in different
    orders and each block must agree to 1e-12 of its largest magnitude (about 3 000 terms at fp64 rounding).  The test prints which holds;
    on the MI355X it is the second for all four objectives: a searched list is summed in the order of the sorted source, an installed one in
    the order it was given (the control differs in the last bits)."""
    pb, ref, eng, masks, E = world["pb"], world["ref"], world["eng"], world["masks"], world["E"]
    P, fx = pb["init"], pb["fixed"]
    roles = T | S
    other = mvicp.Engine(0)
    try:
        other.set_frames(pb["pts"], pb["nor"]); other.set_graph(pb["src"], pb["dst"])
        c0, w0, l0 = unmasked[L.NN_AUTO]
        ref.reset_history(); ref.correspond(P, fx, CUTOFF)
        for e in range(E):
            other.set_correspondences(e, l0[e][0], l0[e][1], w0[e])
        searched, installed = _blocks(ref, P), _blocks(other, P)
        control = {k: (searched[k], installed[k]) for k in searched}
        set_all(eng, masks, roles)
        eng.reset_history()
        counts, weights = eng.correspond(P, fx, CUTOFF)
        want = expected(pb, l0, masks, roles)
        for e in range(E):
            other.set_correspondences(e, want[e][0], want[e][1], want[e][3])
        got, exp = _blocks(eng, P), _blocks(other, P)
        for k in got:
            a, b = control[k]
            exact = a.tobytes() == b.tobytes()
            print("%-9s control %s" % (k, "byte-equal: byte equality demanded" if exact else "differs in summation order: 1e-12 per block demanded"))
            assert np.abs(got[k]).sum() > 0
            if exact:
                assert got[k].tobytes() == exp[k].tobytes(), k
            else:
                for e in range(E):
                    scale = max(np.abs(exp[k][e]).max(), np.abs(got[k][e]).max())
                    assert np.abs(got[k][e] - exp[k][e]).max() <= 1e-12 * scale, (k, e)
        # the queued evaluation (spec_eval) changes nothing under a mask
        poses = {}
        for spec in (1, 0):
            eng.set_option("spec_eval", spec)
            eng.reset_history()
            Q = P.copy()
            for _ in range(4):
                eng.correspond(Q, fx, CUTOFF)
                Q, _ = eng.optimize(Q, fx, L.PARAM_SOPHUS_SE3, True, True, 50)
            poses[spec] = Q
        assert poses[1].tobytes() == poses[0].tobytes() and not np.array_equal(poses[1], P)
    finally:
        eng.set_option("spec_eval", 1)
        set_all(eng, None, 0)
        other.close()


def test_adopt_and_read_back(world):
    import torch
    pb, eng, flags, E = world["pb"], world["eng"], world["flags"], world["E"]
    P, fx = pb["init"], pb["fixed"]
    try:
        assert eng.reject_mask(0) == (None, 0)
        results = {}
        for how in ("numpy", "device", "adopt"):
            for i in range(K):
                if how == "numpy":
                    eng.set_reject_mask(i, flags[i], T | S)
                elif how == "device":
                    eng.set_reject_mask(i, torch.from_numpy(flags[i]).to("cuda:0"), T | S)
                else:
                    assert eng.boundary(i, 30)["flag"].tobytes() == flags[i].tobytes()
                    eng.adopt_boundary_mask(T | S)
                back, roles = eng.reject_mask(i)
                assert back.dtype == np.uint8 and back.tobytes() == flags[i].tobytes() and roles == (T | S), (how, i)
            eng.reset_history()
            c, w = eng.correspond(P, fx, CUTOFF)
            results[how] = (c.tobytes(), w.tobytes(), [tuple(a.tobytes() for a in l) for l in lists(eng, E)])
            set_all(eng, None, 0)
            assert eng.reject_mask(0) == (None, 0)
        assert results["numpy"] == results["device"] == results["adopt"]
        # the bytes come back as they went in (any nonzero byte rejects), and the roles are kept per frame
        odd = np.ascontiguousarray(flags[2] * 7, dtype=np.uint8)
        eng.set_reject_mask(2, odd, S)
        back, roles = eng.reject_mask(2)
        assert back.tobytes() == odd.tobytes() and roles == S and eng.reject_mask(1) == (None, 0)
        eng.reset_history()
        c, w = eng.correspond(P, fx, CUTOFF)
        eng.set_reject_mask(2, flags[2], S)
        eng.reset_history()
        c2, w2 = eng.correspond(P, fx, CUTOFF)
        assert c.tobytes() == c2.tobytes() and w.tobytes() == w2.tobytes()
        eng.adopt_boundary_mask(0)     # roles 0 clears the mask of the last boundary()'s frame (frame 3)
        eng.set_reject_mask(2, None)
    finally:
        set_all(eng, None, 0)


def test_refusals_leave_everything_untouched(world):
    pb, eng, masks, E = world["pb"], world["eng"], world["masks"], world["E"]
    P, fx = pb["init"], pb["fixed"]
    try:
        eng.set_reject_mask(1, masks[1], T)
        eng.reset_history()
        c, w = eng.correspond(P, fx, CUTOFF)
        before, epochs = lists(eng, E), eng.correspondence_epochs()

        def untouched(tag):
            back, roles = eng.reject_mask(1)
            assert back.tobytes() == masks[1].tobytes() and roles == T and eng.reject_mask(0) == (None, 0), tag
            assert eng.correspondence_epochs().tobytes() == epochs.tobytes(), tag
            c2, w2 = eng.correspond(P, fx, CUTOFF)        # the same poses: a search that changes no list, and no epoch
            assert c2.tobytes() == c.tobytes() and w2.tobytes() == w.tobytes() and eng.correspondence_epochs().tobytes() == epochs.tobytes(), tag
            for a, b in zip(before, lists(eng, E)):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), tag

        for frame in (-1, K):
            with pytest.raises(mvicp.MvicpError, match="out of range"):
                eng.set_reject_mask(frame, masks[0], T)
            with pytest.raises(mvicp.MvicpError, match="out of range"):
                eng.set_reject_mask(frame, None)
            untouched(("frame", frame))
        for roles in (-1, 4):
            with pytest.raises(mvicp.MvicpError, match="roles"):
                eng.set_reject_mask(1, masks[0], roles)
            with pytest.raises(mvicp.MvicpError, match="roles"):
                eng.adopt_boundary_mask(roles)
            untouched(("roles", roles))
        with pytest.raises(mvicp.MvicpError):
            eng.set_reject_mask(1, masks[1][:-1], T)      # (the binding's own check: one flag per point)
        untouched("length")
    finally:
        set_all(eng, None, 0)
    # adopt without a boundary result, and after an upload replaced its frame; an upload drops the frame's mask (no graph: uploads are allowed)
    fresh = mvicp.Engine(0)
    try:
        fresh.set_frames(pb["pts"][:2], pb["nor"][:2])
        with pytest.raises(mvicp.MvicpError, match="no boundary result"):
            fresh.adopt_boundary_mask(T)
        assert fresh.reject_mask(0) == (None, 0) and fresh.reject_mask(1) == (None, 0)
        fresh.set_reject_mask(0, masks[0], T | S)
        fresh.set_reject_mask(1, masks[1], T)
        flag = fresh.boundary(0, 30)["flag"]
        fresh.set_frame(0, pb["pts"][0], pb["nor"][0])
        assert fresh.reject_mask(0) == (None, 0)                                   # set_frame dropped the mask ...
        assert fresh.reject_mask(1)[0].tobytes() == masks[1].tobytes()             # ... of that frame only
        with pytest.raises(mvicp.MvicpError, match="no boundary result"):
            fresh.adopt_boundary_mask(T)                                           # ... and the boundary result
        assert fresh.reject_mask(0) == (None, 0)
        fresh.boundary(0, 30)
        fresh.adopt_boundary_mask(S)
        back, roles = fresh.reject_mask(0)
        assert back.tobytes() == flag.tobytes() and roles == S
        fresh.set_frames(pb["pts"][:2], pb["nor"][:2])                              # mvicp_set_num_frames drops every mask
        assert fresh.reject_mask(0) == (None, 0) and fresh.reject_mask(1) == (None, 0)
    finally:
        fresh.close()


@pytest.mark.parametrize("symmetric", [False, True])
def test_registration_of_the_partial_pair_with_the_mask_set_once(symmetric):
    """The 25-round loop of tests/test_gpu_boundary_reject.py with the target's boundary mask set once before the loop and nothing called per
    round.  CPU (tests/test_reject_mask_cpu.py): point-to-plane 0.0469 deg / 0.0713 spacings, symmetric 0.0017 / 0.0032, both closer than
    no rejection (0.0817 / 0.1091, 0.0041 / 0.0083)."""
    metric = L.METRIC_SYMMETRIC if symmetric else L.METRIC_PLANE
    cl = matchref.e2e_clouds(True)
    got = {}
    for reject in (False, True):
        eng = mvicp.Engine(0)
        try:
            eng.set_frames([cl["dst"], cl["src"]], [cl["dst_nrm"], cl["src_nrm"]])
            if reject:
                assert eng.boundary(0, 30, 0.0, -0.5)["boundary"] == 131
                eng.adopt_boundary_mask(T)
            eng.set_graph([1], [0])
            P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
            for _ in range(25):
                eng.correspond(P, [1, 0], 3.0 * cl["spacing"])
                P, _ = eng.optimize_metric(P, [1, 0], L.PARAM_SOPHUS_SE3, metric, True, 50)
        finally:
            eng.close()
        got[reject] = symref.distance_to_truth(P[1], cl["truth"], cl["src"], cl["spacing"])
    a, b = got[False], got[True]
    want = cpu.FIGURES[(True, symmetric)]
    print("GPU partial pair, symmetric=%s: none %.4f deg, %.4f spacings | mask inside the search %.4f deg, %.4f spacings   (CPU: %s, %s)" % (
        (symmetric, a[0], a[1], b[0], b[1]) + want))
    assert ("%.4f" % b[0], "%.4f" % b[1]) == want
    assert ((True, symmetric) in cpu.CLOSER) == (b[0] < a[0] and b[1] < a[1]), got
