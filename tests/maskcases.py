"""Reject masks for the tests of the masked search (TEST INFRASTRUCTURE; include/mvicp.h "reject masks").

Pure, seeded generators (PCG64) of per-point masks -- every one returns a C-contiguous uint8 array, nonzero = reject --, the insertion of
"mask" events into a script of tests/regime_seq.py, and the reference of every masked test: tests/rejectref.py over the lists of a second,
MASKLESS engine run through the same calls (expected_lists), with the hook that drives that engine beside a scripted registration."""
import numpy as np

import rejectref

T, S = 1, 2      # MVICP_REJECT_AS_TARGET, MVICP_REJECT_AS_SOURCE (tests/test_reject_mask_cases_cpu.py holds them to mvicp.lib)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def random_mask(n, p, seed):
    """Every point flagged independently with probability p: the flagged share is within 4 sqrt(p (1 - p) / n) of p, and flagged points sit
    everywhere in any spatial order (no slot of 256 queries and no compaction block is spared or emptied)."""
    return _u8(np.random.Generator(np.random.PCG64(seed)).random(n) < p)


def halfspace_mask(pts, axis, quantile):
    """Flags the points whose coordinate `axis` (the frame's own coordinates) lies above that coordinate's `quantile`: a share of
    1 - quantile (to within one point and ties), contiguous in space -- in any order that sorts by cell, runs of hundreds of flagged points,
    so that whole 256-query dirty slots and whole compaction blocks are rejected."""
    x = np.asarray(pts, dtype=np.float64)[:, axis]
    return _u8(x > np.quantile(x, quantile))


def ones(n):
    """every point flagged: every list the mask bears on is empty"""
    return np.ones(n, dtype=np.uint8)


def zeros(n):
    """a mask that is set and flags nothing: the maskless answer through the masked code path"""
    return np.zeros(n, dtype=np.uint8)


def dup_clouds(pb, seed=11):
    """The recipe of dup_world in tests/test_gpu_search_state.py: a third of every cloud of `pb` appended a second time -> (pts, nor, picks);
    point n0 + j of frame k is a bit copy of point picks[k][j], so every query has both at exactly the same distance."""
    rng = np.random.default_rng(seed)
    pts = [p.copy() for p in pb["pts"]]; nor = [n.copy() for n in pb["nor"]]
    picks = []
    for k in range(len(pts)):
        pick = rng.choice(len(pts[k]), len(pts[k]) // 3, replace=False)
        pts[k] = np.vstack([pts[k], pts[k][pick]]); nor[k] = np.vstack([nor[k], nor[k][pick]])
        picks.append(pick)
    return pts, nor, picks


def duplicate_pair_mask(n0, extra, swap=False):
    """For a cloud of n0 points with point n0 + j a copy of point extra[j]: flags exactly one point of every duplicated pair -- the original
    of every even pair j, the appended copy of every odd one (swap=True: the other way round).  len(extra) points are flagged, and whichever
    of the two a tie rule picks, the other rule's pick of the same pair has the opposite flag."""
    extra = np.asarray(extra, dtype=np.int64)
    m = np.zeros(n0 + len(extra), dtype=np.uint8)
    j = np.arange(len(extra))
    orig = (j % 2 == 0) != bool(swap)
    m[extra[orig]] = 1
    m[n0 + j[~orig]] = 1
    return m


def with_mask_events(events, schedule):
    """schedule: [(index, frame, mask-or-None, roles, tag)].  -> a new list in which a {"kind": "mask"} event stands directly BEFORE the event
    that has `index` in `events` (index = len(events): at the end); entries of one index keep their order.  Every other event is the same
    object in the same order.  The new event takes "param" / "plane" / "robust" (and "metric", if present) from the event it precedes."""
    out = []
    for i in range(len(events) + 1):
        like = events[min(i, len(events) - 1)]
        for (at, frame, mask, roles, tag) in schedule:
            if at == i:
                e = {"kind": "mask", "frame": int(frame), "mask": mask, "roles": int(roles), "tag": tag}
                e.update({k: like[k] for k in ("param", "plane", "robust", "metric") if k in like})
                out.append(e)
        if i < len(events):
            out.append(events[i])
    assert all(0 <= s[0] <= len(events) for s in schedule)
    return out


def standard_masks(n_pts, seed=500):
    """the masks that are on from round 0: 10 % at random on every frame, in both roles -> {frame: (mask, roles)}"""
    return {f: (random_mask(n, 0.1, seed + f), T | S) for f, n in enumerate(n_pts)}


def standard_schedule(events, n_pts, clear=False, seed=900):
    """The mask changes of the scripted tests, placed by the script's own kinds:
      "after_hold"   a new random mask on frame 2 in the round directly after the first "hold": the fixed point's shortcuts were live;
      "before_solve" a new random mask on the last frame as SOURCE between two rounds that both solve: the first one's solve has armed the
                     queued evaluation of the next search when the mask changes;
      "ones"         all-ones on frame 1 as TARGET in the middle of the script, "restore" (its round-0 mask, both roles) two events later;
      "clear"        (clear=True) frame 2's mask cleared before event 3."""
    K = len(n_pts)
    kinds = [e["kind"] for e in events]
    solve = [k not in ("hold", "fail") for k in kinds]
    i_hold = kinds.index("hold") + 1
    i_solve = next(i for i in range(1, len(kinds)) if solve[i - 1] and solve[i] and i != i_hold)
    i_ones = len(kinds) // 2
    sched = [(i_hold, 2, random_mask(n_pts[2], 0.1, seed), T | S, "after_hold"),
             (i_solve, K - 1, random_mask(n_pts[K - 1], 0.15, seed + 1), S, "before_solve"),
             (i_ones, 1, ones(n_pts[1]), T, "ones"),
             (i_ones + 2, 1, standard_masks(n_pts)[1][0], T | S, "restore")]
    if clear:
        sched.append((3, 2, None, 0, "clear"))
    return sched


def expected_lists(pb, ref_lists, masks_and_roles):
    """rejectref over the MASKLESS engine's lists.  ref_lists: per edge (first, second, dist); masks_and_roles: per frame (a list or a dict)
    (mask or None, roles) -> per edge (first, second, dist, weight) of the masked search."""
    out = []
    for e, (f, s, d) in enumerate(ref_lists):
        ms, rs = masks_and_roles[int(pb["src"][e])]
        md, rd = masks_and_roles[int(pb["dst"][e])]
        out.append(rejectref.masked(f, s, d, ms if (rs & S) else None, md if (rd & T) else None))
    return out


def assert_lists(got_lists, counts, weights, want, tag, edges=None):
    """lists, counts and weight bits of the edges (default: all) equal `want`, byte for byte"""
    for e in (range(len(want)) if edges is None else edges):
        (gf, gs, gd), (wf, ws, wd, ww) = got_lists[e], want[e]
        assert counts[e] == len(wf), (tag, e, int(counts[e]), len(wf))
        assert gf.tobytes() == wf.tobytes() and gs.tobytes() == ws.tobytes() and gd.tobytes() == wd.tobytes(), (tag, e)
        assert np.float32(weights[e]).tobytes() == np.float32(ww).tobytes(), (tag, e, weights[e], ww)


def lists(eng, E):
    return [eng.get_correspondences(e) for e in range(E)]


def anchor_hook(eng, ref, pb, seen=None, extra=None):
    """-> an after_search hook for regime_seq.run(eng, ...): the maskless engine `ref` takes the round's option, tie-rule and reset events and
    then the round's OWN search (never a scripted failing one) at the same poses, fixed flags, cutoff and method; the masked engine's lists,
    counts and weights must equal expected_lists over ref's lists under state["masks"].  extra(state, ref_counts), if given, runs after the check;
    seen["searches"] counts the checks."""
    E = len(pb["src"])
    rule = {"value": 1}

    def hook(st):
        e = st["event"]
        if e["kind"] == "option":
            ref.set_option(e["name"], e["value"])
        elif e["kind"] == "tie_rule":
            rule["value"] = 1 - rule["value"]
            ref.set_option("tie_rule", rule["value"])
        elif e["kind"] == "reset":
            ref.reset_history()
        rc, rw = ref.correspond(st["poses"], st["fixed"], st["cutoff"], st["method"])
        want = expected_lists(pb, lists(ref, E), st["masks"])
        assert_lists(lists(eng, E), st["counts"], st["weights"], want, ("round", st["round"], e["kind"], e.get("tag")))
        if seen is not None:
            seen["searches"] = seen.get("searches", 0) + 1
        if extra is not None:
            extra(st, rc)
    return hook
