"""-m gpu: reject masks on 2 and 4 ranks that share GPU 0 (the harness of tests/test_gpu_multirank.py: host-staged transport over gloo).

Every rank builds the same masks (tests/maskcases.py: seeded, nothing is communicated), sets them before the same search and replays the same
script of tests/regime_seq.py with mask changes in it -- after a "hold", between two solves, to all-ones on one frame (its owner then
contributes zeros to the exchanged counts and medians), back, and a clear.  mvicp's reject_mask_changed walks the edges a rank OWNS; counts and
medians are exchanged; the queued evaluations go through the exchange.  After every round each rank's counts, weight bits and poses equal the
single process's bit for bit, the lists a rank owns equal the single process's, and the queued evaluation is served as often.  The single
process itself is held, after every search, to a MASKLESS engine + tests/rejectref.py (maskcases.anchor_hook): the sharded answer is
anchored to the reference, not only to another run of the code under test."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 5


def _paths():
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _masked_run(rank, world, allreduce, seed, spec, metrics, anchor=False):
    """-> (events, log, spec.hit, {round: {edge: (first, second, dist)}} of the edges this rank owns, after the round that follows the
    all-ones event and after the last round)"""
    import maskcases
    import mvicp
    import regime_seq
    import test_gpu_multirank as mr
    from mvicp import lib as L
    pb = mr._regime_problem(seed)
    n_pts = [len(p) for p in pb["pts"]]
    eng = mvicp.Engine(0, rank=rank, world=world)
    ref = mvicp.Engine(0) if anchor else None
    try:
        eng.set_option("spec_eval", spec)
        eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
        if allreduce is not None:
            eng.comm_set_callback(allreduce)
        eng.profile(True)
        base = regime_seq.script(seed, FRAMES, extended=seed >= 100, metrics=metrics)
        events = maskcases.with_mask_events(base, maskcases.standard_schedule(base, n_pts, clear=True))
        masks = maskcases.standard_masks(n_pts)
        for f, (m, r) in masks.items():
            eng.set_reject_mask(f, m, r)
        own = L.edge_owner([n_pts[s] for s in pb["src"]], world)
        mine = [e for e in range(len(pb["src"])) if own[e] == rank]
        after_ones = [i for i, e in enumerate(events) if e.get("tag") == "ones"][0] + 1
        saved = {}
        trace = []      # per round, cumulative: evaluations served from the queue, launches of the median select

        def after_round(st):
            trace.append((int(eng.profile_get("spec.hit")[1]), int(eng.profile_get("select")[1])))
            if st["round"] in (after_ones, len(events) - 1):
                saved[st["round"]] = {e: eng.get_correspondences(e) for e in mine}

        hook = None
        seen = {}
        if anchor:
            ref.set_frames(pb["pts"], pb["nor"]); ref.set_graph(pb["src"], pb["dst"])
            hook = maskcases.anchor_hook(eng, ref, pb, seen)
        log = regime_seq.run(eng, pb, events, after_search=hook, after_round=after_round, masks=masks)
        assert not anchor or seen["searches"] == len(events)
        hits = eng.profile_get("spec.hit")[1]
    finally:
        eng.close()
        if ref is not None:
            ref.close()
    return events, log, hits, saved, trace


def _worker(rank, world, port, out, seed, spec, metrics):
    _paths()
    import regime_seq
    import test_gpu_multirank as mr
    allreduce = mr._group(rank, world, port, seconds=120)
    _, log, hits, saved, trace = _masked_run(rank, world, allreduce, seed, spec, metrics)
    regime_seq.save(f"{out}.{rank}.npz", log)
    np.save(f"{out}.{rank}.hits.npy", np.array([hits]))
    np.save(f"{out}.{rank}.trace.npy", np.array(trace))
    flat = {}
    for rnd, per_edge in saved.items():
        for e, (f, s, d) in per_edge.items():
            flat[f"{rnd}_{e}_first"] = f; flat[f"{rnd}_{e}_second"] = s; flat[f"{rnd}_{e}_dist"] = d
    np.savez(f"{out}.{rank}.lists.npz", **flat)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("seed,spec,world,metrics", [(0, 1, 2, True), (1, 0, 2, False), (100, 1, 2, False), (2, 1, 4, False)])
def test_masked_regime_script_sharded_matches_the_single_process(tmp_path, seed, spec, world, metrics):
    """metrics=True: the objective of every solve is drawn from {POINT, PLANE, SYMMETRIC}: every objective reads the filtered list, sharded too.

    The last assertion -- every rank serves as many evaluations from the queue as the single process -- found a fault of the planner, not of the
    masks: the one-pass bracket select was armed per rank, when every active edge OF THAT RANK had a settled median.  After the "after_hold"
    mask change, which unsettles the edges that touch frame 2, the ranks of case (2, 1, 4) that own none of them armed a bracket the single
    process did not; the next medians left it, every rank ran the select a second time (redo_select, with a second exchange) and dropped
    its queued evaluation: 3 served per rank against 4.  plan_search now asks the exchanged medians of every searched edge
    (csrc/search_plan.h; tests/test_search_plan_cpu.py); the printed table shows the select launches per round beside the single process's."""
    _paths()
    import regime_seq
    import test_gpu_multirank as mr
    from mvicp import lib as L
    out = str(tmp_path / "masked")
    mp.spawn(_worker, args=(world, mr._free_port(), out, seed, spec, metrics), nprocs=world, join=True)
    events, log, hits1, saved, trace1 = _masked_run(0, 1, None, seed, spec, metrics, anchor=True)
    traces = [np.load(f"{out}.{r}.trace.npy") for r in range(world)]
    print("round kind         tag           | cumulative (spec.hit, select launches): single process | per rank")
    for i, e in enumerate(events):
        print("%5d %-12s %-13s | %s | %s" % (i, e["kind"], e.get("tag", ""), trace1[i], [tuple(t[i]) for t in traces]))
    kinds = [e["kind"] for e in events]
    assert kinds.count("mask") == 5 and len(set(kinds)) >= 5, kinds
    if seed >= 100:
        assert "fail" in kinds and "tie_rule" in kinds, kinds
    if metrics:
        assert [e["metric"] for e in regime_seq.solves(events)].count(2) >= 3
    pb = mr._regime_problem(seed)
    own = L.edge_owner([len(pb["pts"][s]) for s in pb["src"]], world)
    assert sorted(set(own.tolist())) == list(range(world)), own
    # the round after the all-ones event: the edges into frame 1 are empty, and some rank owns one
    ones_round = min(saved)
    into1 = [e for e in range(len(pb["src"])) if pb["dst"][e] == 1]
    assert into1 and all(len(saved[ones_round][e][0]) == 0 for e in into1) and not log[ones_round][0][into1].any()
    assert any(len(saved[ones_round][e][0]) > 0 for e in saved[ones_round])
    if spec:
        assert hits1 > 0                  # a mask does not turn the queued evaluation off
    else:
        assert hits1 == 0
    checked = 0
    for r in range(world):
        regime_seq.assert_equal(f"{out}.{r}.npz", log, (seed, spec, world, r, kinds))
        z = np.load(f"{out}.{r}.lists.npz")
        mine = [e for e in range(len(own)) if own[e] == r]
        assert sorted(z.files) == sorted(f"{rnd}_{e}_{k}" for rnd in saved for e in mine for k in ("first", "second", "dist")), (r, z.files)
        for rnd in saved:
            for e in mine:
                f, s, d = saved[rnd][e]
                assert z[f"{rnd}_{e}_first"].tobytes() == f.tobytes() and z[f"{rnd}_{e}_second"].tobytes() == s.tobytes() and z[f"{rnd}_{e}_dist"].tobytes() == d.tobytes(), (r, rnd, e)
                checked += 1
    assert checked == 2 * len(own)
    # the queued evaluation is served as often as in the single process (last: everything above is checked whatever this finds)
    hits = [int(np.load(f"{out}.{r}.hits.npy")[0]) for r in range(world)]
    assert hits == [int(hits1)] * world, (hits, int(hits1))
