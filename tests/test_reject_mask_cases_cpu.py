"""No GPU: the mask generators of tests/maskcases.py are deterministic and have the properties their docstrings state, with_mask_events leaves
the scripts of tests/regime_seq.py as they were drawn, and the INPUT CONDITIONS of the GPU tests that use them hold on the CPU reference alone
(tests/cpupath.py: the oracle and the real nanoflann): the tie case of tests/test_gpu_reject_mask_paths.py has queries whose two tie rules pick
differently flagged copies, in both directions, and its bracket case moves a median by more than the one-pass select's bracket."""
import numpy as np
import pytest

import cpupath
import maskcases
import regime_seq
import rejectref
import test_regime_script_cpu as digests
from mvicp import lib as L
from mvicp import synth

CUTOFF = 0.05
PATH_SCRIPTS = [(0, False), (1, False), (100, True), (2, False)]        # tests/test_gpu_reject_mask_paths.py, 4 frames
SHARDED_SCRIPTS = [(0, True), (1, False), (100, False), (2, False)]     # tests/test_gpu_reject_mask_sharded.py, 5 frames: (seed, metrics)


def test_the_role_bits_are_the_librarys():
    assert (maskcases.T, maskcases.S) == (L.REJECT_AS_TARGET, L.REJECT_AS_SOURCE)


def _cell_order(pts, axis):
    """np.lexsort over cell-sized bins (cell = extent / cbrt(n), the first estimate of the library's grid), `axis` the slowest key"""
    ext = float((pts.max(axis=0) - pts.min(axis=0)).max())
    b = np.floor((pts - pts.min(axis=0)) / (ext / np.cbrt(len(pts)))).astype(np.int64)
    others = [a for a in range(3) if a != axis]
    return np.lexsort((b[:, others[0]], b[:, others[1]], b[:, axis]))


def _longest_run(flags):
    best = run = 0
    for v in flags:
        run = run + 1 if v else 0
        best = max(best, run)
    return best


def test_generators_are_deterministic_and_have_their_stated_properties():
    pb = synth.make_problem(4, 3000)
    for n, p, seed in ((3000, 0.1, 1), (3500, 0.15, 2), (4000, 0.5, 3)):
        m = maskcases.random_mask(n, p, seed)
        assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and m.shape == (n,) and set(np.unique(m)) <= {0, 1}
        assert m.tobytes() == maskcases.random_mask(n, p, seed).tobytes() and m.tobytes() != maskcases.random_mask(n, p, seed + 1).tobytes()
        assert abs(m.mean() - p) <= 4.0 * np.sqrt(p * (1 - p) / n), (n, p, m.mean())
        slots = m[: n // 256 * 256].reshape(-1, 256).sum(axis=1)
        assert (slots > 0).all() and (slots < 256).all()                       # no slot of 256 is spared or emptied
    for f in range(4):
        for axis in range(3):
            for q in (0.5, 0.7):
                m = maskcases.halfspace_mask(pb["pts"][f], axis, q)
                assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and m.shape == (3000,)
                assert m.tobytes() == maskcases.halfspace_mask(pb["pts"][f], axis, q).tobytes()
                assert abs(int(m.sum()) - round((1 - q) * 3000)) <= 1, (f, axis, q, int(m.sum()))
                run = _longest_run(m[_cell_order(pb["pts"][f], axis)])
                assert run >= 256, (f, axis, q, run)
    assert maskcases.ones(7).tobytes() == b"\x01" * 7 and maskcases.zeros(7).tobytes() == b"\x00" * 7
    assert maskcases.ones(7).dtype == maskcases.zeros(7).dtype == np.uint8


def test_duplicate_pair_mask_flags_one_point_of_every_pair():
    extra = np.array([5, 2, 9, 0, 7])
    m = maskcases.duplicate_pair_mask(10, extra)
    assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and m.tolist() == [0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    w = maskcases.duplicate_pair_mask(10, extra, swap=True)
    j = np.arange(5)
    assert ((m[extra] + m[10 + j]) == 1).all() and ((w[extra] + w[10 + j]) == 1).all() and ((m[extra] + w[extra]) == 1).all()
    assert int(m.sum()) == int(w.sum()) == 5


@pytest.mark.parametrize("seed,K,extended,metrics", [(s, 4, x, False) for s, x in PATH_SCRIPTS] + [(s, 5, s >= 100, m) for s, m in SHARDED_SCRIPTS])
def test_with_mask_events_leaves_the_script_as_it_was_drawn(seed, K, extended, metrics):
    base = regime_seq.script(seed, K, extended=extended, metrics=metrics)
    n_pts = [3000] * K
    sched = maskcases.standard_schedule(base, n_pts, clear=(K == 5))
    events = maskcases.with_mask_events(base, sched)
    rest = [e for e in events if e["kind"] != "mask"]
    assert len(rest) == len(base) and all(a is b for a, b in zip(rest, base))
    assert rest == regime_seq.script(seed, K, extended=extended, metrics=metrics)          # (nothing was written into them either)
    if K == 5 and seed in digests.DIGESTS:
        assert digests._digest([{k: v for k, v in e.items() if k != "metric"} for e in rest]) == digests.DIGESTS[seed]
    added = [e for e in events if e["kind"] == "mask"]
    assert [e["tag"] for e in added if e["tag"] != "clear"].count("ones") == 1 and len(added) == len(sched)
    assert all(("metric" in e) == metrics and {"param", "plane", "robust"} <= set(e) for e in added)
    tag_at = {e["tag"]: i for i, e in enumerate(events) if e["kind"] == "mask"}
    solves = lambda e: e["kind"] not in ("hold", "fail")
    # where the schedule says its changes stand
    i = tag_at["after_hold"]
    assert events[i - 1]["kind"] == "hold" or (events[i - 1]["kind"] == "mask" and events[i - 2]["kind"] == "hold")
    i = tag_at["before_solve"]
    assert solves(events[i - 1]) and events[i - 1]["kind"] != "mask" and i + 1 < len(events) and solves(events[i + 1])
    assert tag_at["ones"] < tag_at["restore"] and any(e["kind"] != "mask" for e in events[tag_at["ones"] + 1:tag_at["restore"]])
    assert events[tag_at["ones"]]["roles"] == maskcases.T and events[tag_at["ones"]]["mask"].all()
    assert events[tag_at["restore"]]["mask"].tobytes() == maskcases.standard_masks(n_pts)[1][0].tobytes()
    if K == 5:
        assert events[tag_at["clear"]]["mask"] is None


def test_the_scripts_hold_the_kinds_the_gpu_tests_are_about():
    """No script of seeds 0, 1, 100 draws a "method" event: seed 2 is run beside them for it."""
    kinds = {s: {e["kind"] for e in regime_seq.script(s, 4, extended=x)} for s, x in PATH_SCRIPTS}
    union = set().union(*kinds.values())
    assert {"method", "option", "reset", "hold", "cutoff", "fixed"} <= union, union
    assert {"fail", "tie_rule"} <= kinds[100] and "method" in kinds[2] and "option" in kinds[0] and all("reset" in k for k in kinds.values())
    m = [e["metric"] for e in regime_seq.solves(regime_seq.script(0, 5, metrics=True))]
    assert m.count(2) >= 3 and m.count(1) >= 3 and any(a == 2 and b == 1 for a, b in zip(m, m[1:])), m      # the sharded symmetric case


def test_tie_case_input_condition(orc, refnn):
    """The duplicated clouds at the ground-truth poses, rule 1 = the real nanoflann, rule 0 = the oracle's lowest index: there are queries
    whose neighbour differs between the rules and where exactly one of the two picks is flagged by duplicate_pair_mask, in both directions
    -- so the masked lists of the two rules differ in `first`, not only in `second`."""
    assert refnn is not None, "oracle/_ref (real nanoflann) was not built"
    pb = synth.make_problem(3, 3000)
    pts, nor, picks = maskcases.dup_clouds(pb)
    masks = [maskcases.duplicate_pair_mask(3000, picks[k]) for k in range(3)]
    P0 = pb["gt"]
    cpu = cpupath.CpuPath(pts, nor, pb["src"], pb["dst"], pb["fixed"], 2, 1, orc=orc, ref=refnn)
    nano = cpu.correspond(P0)
    cpu.close()
    only0 = only1 = 0
    for e in range(len(pb["src"])):
        s, d = pb["src"][e], pb["dst"][e]
        f1, s1, d1, _ = nano[e]
        f0, s0, d0 = orc.correspond_edge(pts[s], P0[s], pts[d], P0[d], CUTOFF)[:3]
        assert np.array_equal(f0, f1) and d0.tobytes() == d1.tobytes()             # a tie: the same distance whichever copy is picked
        differ = s0 != s1
        a, b = masks[d][s0] != 0, masks[d][s1] != 0
        n0, n1 = int((differ & a & ~b).sum()), int((differ & ~a & b).sum())
        only0 += n0; only1 += n1
        k0 = rejectref.masked(f0, s0, d0, None, masks[d])[0]
        k1 = rejectref.masked(f1, s1, d1, None, masks[d])[0]
        if n0 + n1:
            assert k0.tobytes() != k1.tobytes(), e
    print("queries whose picks differ with only rule 0's flagged: %d, only rule 1's: %d" % (only0, only1))
    assert only0 > 0 and only1 > 0, (only0, only1)


BRACKET = {"frame": 2, "axis": 0, "quantile": 0.5}     # the halfspace mask of the bracket case (tests/test_gpu_reject_mask_paths.py)


def median_shift(pb, ref_lists, before, after):
    """per edge: relative change of the upper median's SQUARED distance between two mask settings, from the maskless lists alone (nan: an empty list)"""
    out = []
    for (_, _, da, _), (_, _, db, _) in zip(maskcases.expected_lists(pb, ref_lists, before), maskcases.expected_lists(pb, ref_lists, after)):
        if len(da) == 0 or len(db) == 0:
            out.append(float("nan")); continue
        ma, mb = np.sort(da)[len(da) // 2] ** 2, np.sort(db)[len(db) // 2] ** 2
        out.append(float(abs(mb - ma) / ma))
    return out


def test_bracket_case_input_condition(orc, refnn):
    """At the initial poses the halfspace mask on a source frame moves the upper median of an edge out of that frame by more than the
    +-0.6 % (in squared distance) that the one-pass select brackets around the last median."""
    pb = synth.make_problem(4, 3000)
    cpu = cpupath.CpuPath(pb["pts"], pb["nor"], pb["src"], pb["dst"], pb["fixed"], 2, 1, orc=orc, ref=refnn)
    ref_lists = [c[:3] for c in cpu.correspond(pb["init"])]
    cpu.close()
    before = maskcases.standard_masks([3000] * 4)
    after = dict(before)
    after[BRACKET["frame"]] = (maskcases.halfspace_mask(pb["pts"][BRACKET["frame"]], BRACKET["axis"], BRACKET["quantile"]), maskcases.S)
    shift = median_shift(pb, ref_lists, before, after)
    print("relative change of the median d2 per edge:", ["%.4f" % s for s in shift])
    out_of = [e for e in range(len(pb["src"])) if pb["src"][e] == BRACKET["frame"]]
    assert out_of and max(shift[e] for e in out_of) > 0.006, shift
