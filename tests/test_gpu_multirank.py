"""-m gpu: the N > 1 DEVICE path on a one-GPU box — `world` processes share GPU 0, each owns its shard of the edges and runs
the real kernels; the exchanged buffer ([queued blocks | counts | medians | armed | scales] per search, the per-edge blocks per LM
evaluation) goes through the host-staged callback (gloo) instead of RCCL (RCCL refuses two ranks on one device) — the same code path
in api.cpp as the RCCL one up to the transport call.  Poses, counts and weights must be bit-identical to the single-process run for
world = 2, 4 and 8 (62 -> 7-8 edges per rank on config 4; here 18 edges over up to 8 ranks)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 8


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run(rank, world, reduce_fn, spec=1):
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    import mvicp
    from mvicp import synth
    pb = synth.make_problem(10, 4000)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_option("spec_eval", spec)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    if reduce_fn is not None:
        eng.comm_set_callback(reduce_fn)
    eng.profile(True)
    poses = pb["init"].copy()
    hist = []
    for _ in range(ROUNDS):
        c, w = eng.correspond(poses, pb["fixed"], 0.05)
        poses, sm = eng.optimize(poses, pb["fixed"])
        hist.append((c.copy(), w.copy(), sm["iterations"], sm["evaluations"]))
    hits = eng.profile_get("spec.hit")[1]
    comms = eng.profile_get("comm")[1]
    eng.close()
    return poses, hist, hits, comms


def _worker(rank, world, port, out, spec):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce(a):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)

    poses, hist, hits, comms = _run(rank, world, allreduce, spec)
    np.save(f"{out}.{rank}.npy", poses)
    np.save(f"{out}.{rank}.counts.npy", np.array([h[0] for h in hist]))
    np.save(f"{out}.{rank}.meta.npy", np.array([hits, comms, sum(h[3] for h in hist)]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,spec", [(2, 1), (2, 0), (4, 1), (8, 1)])
def test_ranks_on_one_gpu_match_single_process_bitwise(tmp_path, world, spec):
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    from mvicp import lib as L
    from mvicp import synth
    out = str(tmp_path / "poses")
    mp.spawn(_worker, args=(world, _free_port(), out, spec), nprocs=world, join=True)
    P1, hist, hits1, _ = _run(0, 1, None, spec)
    assert hist[-1][2] >= 1
    for r in range(world):
        P2 = np.load(f"{out}.{r}.npy")
        assert np.array_equal(P1, P2), (r, np.abs(P1 - P2).max())
        assert np.array_equal(np.load(f"{out}.{r}.counts.npy"), np.array([h[0] for h in hist]))   # every rank holds the global counts
        hits, comms, evals = np.load(f"{out}.{r}.meta.npy")
        assert hits == hits1 == (ROUNDS - 1 if spec else 0), (r, hits, hits1)                     # the queued evaluation is served on every rank
        assert comms == ROUNDS + evals - hits, (r, comms, evals, hits)                            # one exchange per search + one per evaluated LM step
    # partition: contiguous, balanced by source points (mvicp_edge_owner)
    pb = synth.make_poses(10)
    own = L.edge_owner([4000] * len(pb["src"]), world)
    assert np.all(np.diff(own) >= 0) and own[0] == 0 and own[-1] == world - 1
    sizes = np.bincount(own, minlength=world)
    assert sizes.max() - sizes.min() <= 1, sizes


def test_partition_of_config4_and_config5_over_8_ranks():
    """62 edges -> 7-8 per rank, 126 -> 15-16 per rank, contiguous chunks."""
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    from mvicp import lib as L
    for E, lo, hi in ((62, 7, 8), (126, 15, 16)):
        own = L.edge_owner([200000] * E, 8)
        sizes = np.bincount(own, minlength=8)
        assert sizes.min() >= lo and sizes.max() <= hi and np.all(np.diff(own) >= 0), sizes


# ---------------------------------------------------------------- regime transitions, sharded
def _regime_worker(rank, world, port, out, seed, spec):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mvicp
    import regime_seq
    from mvicp import synth

    def allreduce(a):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)

    pb = synth.make_problem(5, 3500, cone_deg=100.0 if seed % 2 == 0 else 45.0, pose_seed=800 + seed)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_option("spec_eval", spec)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    eng.comm_set_callback(allreduce)
    log = regime_seq.run(eng, pb, regime_seq.script(seed, 5, extended=seed >= 100))
    eng.close()
    regime_seq.save(f"{out}.{rank}.npz", log)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("seed,spec", [(0, 1), (1, 1), (2, 0), (3, 1), (100, 1)])   # seeds >= 100: extended scripts (failed searches, tie-rule flips)
def test_regime_transitions_sharded_match_single_process(tmp_path, seed, spec):
    """mvicp_correspond's cross-round state (tie_skip / far_skip / spec_arm / bracket select / list reuse / AUTO policy) under a scripted
    registration that changes the cutoff, the fixed mask, the kernel method and options, resets the history and repeats poses — on TWO ranks
    sharing the edges (host-staged transport): after EVERY round each rank's counts, float weights and poses equal the single process's bit for
    bit, with the queued first evaluation on (spec 1) and off (spec 0)."""
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mvicp
    import regime_seq
    from mvicp import synth
    out = str(tmp_path / "regime")
    mp.spawn(_regime_worker, args=(2, _free_port(), out, seed, spec), nprocs=2, join=True)
    pb = synth.make_problem(5, 3500, cone_deg=100.0 if seed % 2 == 0 else 45.0, pose_seed=800 + seed)
    eng = mvicp.Engine(0)
    eng.set_option("spec_eval", spec)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    events = regime_seq.script(seed, 5, extended=seed >= 100)
    log = regime_seq.run(eng, pb, events)
    eng.close()
    kinds = [e["kind"] for e in events]
    if seed >= 100:
        assert "fail" in kinds and "tie_rule" in kinds, kinds
    assert len(set(kinds)) >= 4, kinds                                  # the script really mixes events
    for r in range(2):
        regime_seq.assert_equal(f"{out}.{r}.npz", log, (seed, spec, r, kinds))


# ---------------------------------------------------------------- a rank that fails locally must not leave its peers in the collective
def _fault_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    import mvicp
    from mvicp import synth

    def allreduce(a):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)

    pb = synth.make_problem(6, 3000)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    eng.comm_set_callback(allreduce)
    poses = pb["init"].copy()
    log = []
    for rnd in range(7):
        if rnd == 2 and rank == 1:
            eng.set_option("fault_inject", 1)        # THIS rank's next search fails before the search's collective
        if rnd == 4 and rank == 0:
            eng.set_option("fault_inject_eval", 1)   # this rank's next exchanged LM evaluation fails before ITS collective
        try:
            c, w = eng.correspond(poses, pb["fixed"], 0.05)
        except mvicp.MvicpError as ex:
            log.append((rnd, "correspond", str(ex)))
            c, w = eng.correspond(poses, pb["fixed"], 0.05)      # the retry is a first search on every rank
        try:
            poses, sm = eng.optimize(poses, pb["fixed"])
        except mvicp.MvicpError as ex:
            log.append((rnd, "optimize", str(ex)))
    eng.close()
    np.save(f"{out}.{rank}.npy", poses)
    with open(f"{out}.{rank}.log", "w") as f:
        for r in log:
            f.write("%d|%s|%s\n" % r)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_local_failure_reaches_every_rank_through_the_collective(tmp_path):
    """VERDICT r4 item 7 / ADVICE r3: a rank whose search (or LM evaluation) fails locally before the exchange still enters the collective,
    with the exchanged buffer poisoned; EVERY rank returns an error from that same call (the failing rank its own, the peers MVICP_ERR_COMM)
    within the timeout instead of blocking forever, every rank drops its cross-round state, and the job goes on: the retried search and
    the rounds after it agree bit for bit across ranks and with a single process that reset its history at the same point."""
    out = str(tmp_path / "fault")
    mp.spawn(_fault_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    logs = [[l.rstrip("\n").split("|", 2) for l in open(f"{out}.{r}.log")] for r in range(2)]
    for r in range(2):
        assert [(int(a), b) for a, b, _ in logs[r]] == [(2, "correspond"), (4, "optimize")], logs[r]
    assert "injected launch failure" in logs[1][0][2] and "peer rank failed" in logs[0][0][2], (logs[0][0], logs[1][0])
    assert "injected launch failure" in logs[0][1][2] and "peer rank failed" in logs[1][1][2], (logs[0][1], logs[1][1])
    P0, P1 = np.load(f"{out}.0.npy"), np.load(f"{out}.1.npy")
    assert np.array_equal(P0, P1)
    # single process: the same rounds, history dropped where the failed search dropped it, round 4's solve skipped (it failed on both ranks)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    import mvicp
    from mvicp import synth
    pb = synth.make_problem(6, 3000)
    eng = mvicp.Engine(0)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    poses = pb["init"].copy()
    for rnd in range(7):
        if rnd == 2:
            eng.reset_history()
        eng.correspond(poses, pb["fixed"], 0.05)
        if rnd == 4:
            continue
        poses, _ = eng.optimize(poses, pb["fixed"])
    eng.close()
    assert np.array_equal(P0, poses), np.abs(P0 - poses).max()


# ---------------------------------------------------------------- the symmetric objective, sharded
def _group(rank, world, port, seconds=120):
    """a process group whose collectives give up after `seconds`: a rank left alone in one ends as an exception, not as a blocked test"""
    import datetime
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=seconds))

    def allreduce(a):
        t = torch.from_numpy(a)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return allreduce


def _regime_problem(seed):
    from mvicp import synth
    return synth.make_problem(5, 3500, cone_deg=100.0 if seed % 2 == 0 else 45.0, pose_seed=800 + seed)


def _regime_metric_run(rank, world, allreduce, seed, spec):
    """-> (events, log, spec.hit) of the script with a metric per solve"""
    import mvicp
    import regime_seq
    pb = _regime_problem(seed)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_option("spec_eval", spec)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    if allreduce is not None:
        eng.comm_set_callback(allreduce)
    eng.profile(True)
    events = regime_seq.script(seed, 5, extended=seed >= 100, metrics=True)
    log = regime_seq.run(eng, pb, events)
    hits = eng.profile_get("spec.hit")[1]
    eng.close()
    return events, log, hits


def _regime_metric_worker(rank, world, port, out, seed, spec):
    allreduce = _group(rank, world, port)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import regime_seq
    _, log, hits = _regime_metric_run(rank, world, allreduce, seed, spec)
    regime_seq.save(f"{out}.{rank}.npz", log)
    np.save(f"{out}.{rank}.hits.npy", np.array([hits]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("seed,spec", [(4, 1), (5, 0), (125, 1)])   # chosen on the CPU (regime_seq.script, metrics=True) for the mix asserted below; 125: extended
def test_regime_transitions_sharded_symmetric_match_single_process(tmp_path, seed, spec):
    """The scripted registration of the test above with the objective of every solve drawn from {POINT, PLANE, SYMMETRIC} (mvicp_optimize_metric), on
    TWO ranks: the symmetric evaluations go through the exchange branch of evaluate_blocks (extended-precision relative transforms uploaded before
    the collective, no normals gathered for the peer's edges), between solves of the other objectives that arm and consume the queued evaluation.
    After EVERY round each rank's counts, weight bits and poses equal the single process's bit for bit, and so does the number of evaluations
    served from the queue."""
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import regime_seq
    out = str(tmp_path / "regime_sym")
    mp.spawn(_regime_metric_worker, args=(2, _free_port(), out, seed, spec), nprocs=2, join=True)
    events, log, hits1 = _regime_metric_run(0, 1, None, seed, spec)
    kinds = [e["kind"] for e in events]
    m = [e["metric"] for e in regime_seq.solves(events)]
    assert m.count(2) >= 3, m
    assert any(a == 1 and b == 2 for a, b in zip(m, m[1:])) and any(a == 2 and b == 1 for a, b in zip(m, m[1:])), m   # symmetric right after plane, and plane right after symmetric
    assert len(set(kinds)) >= 4, kinds
    if seed >= 100:
        assert "fail" in kinds and "tie_rule" in kinds, kinds
    assert all(l[0].sum() > 0 for l in log)          # every round that the script lets solve did solve
    if not spec:
        assert hits1 == 0
    for r in range(2):
        regime_seq.assert_equal(f"{out}.{r}.npz", log, (seed, spec, r, kinds, m))
        assert np.load(f"{out}.{r}.hits.npy")[0] == hits1, (r, hits1)


FAULT_METRICS = [1, 2, 2, 1, 2]     # per round; the solve of round 2 (SYMMETRIC) fails on rank 1


def _fault_sym_rounds(eng, pb, rank, skip_round2):
    import mvicp
    poses = pb["init"].copy()
    log, errors = [], []
    for rnd, metric in enumerate(FAULT_METRICS):
        c, w = eng.correspond(poses, pb["fixed"], 0.05)
        if rnd == 2 and rank == 1:
            eng.set_option("fault_inject_eval", 1)   # this rank's next exchanged evaluation fails after the symmetric upload, before the collective
        if not (rnd == 2 and skip_round2):
            try:
                poses, _ = eng.optimize_metric(poses, pb["fixed"], mvicp.lib.PARAM_SOPHUS_SE3, metric, True, 50)
            except mvicp.MvicpError as ex:
                errors.append((rnd, str(ex)))
        log.append((c.copy(), w.tobytes(), poses.copy()))
    return log, errors


def _fault_sym_worker(rank, world, port, out):
    allreduce = _group(rank, world, port)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mvicp
    import regime_seq
    from mvicp import synth
    pb = synth.make_problem(5, 2000)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    eng.comm_set_callback(allreduce)
    log, errors = _fault_sym_rounds(eng, pb, rank, False)
    eng.close()
    regime_seq.save(f"{out}.{rank}.npz", log)
    with open(f"{out}.{rank}.log", "w") as f:
        for r in errors:
            f.write("%d|%s\n" % r)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_local_failure_in_a_symmetric_evaluation_reaches_every_rank(tmp_path):
    """The LM leg of the test above for the symmetric objective: rank 1's first evaluation of a symmetric solve fails locally (after upload_rel_sym,
    before the collective).  Both ranks return an error from that mvicp_optimize_metric — rank 1 its own, rank 0 MVICP_ERR_COMM — and the
    rounds after it (plane, then symmetric again) agree bit for bit across ranks and with a single process that skipped that solve."""
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mvicp
    import regime_seq
    from mvicp import synth
    out = str(tmp_path / "fault_sym")
    mp.spawn(_fault_sym_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    logs = [[l.rstrip("\n").split("|", 1) for l in open(f"{out}.{r}.log")] for r in range(2)]
    for r in range(2):
        assert [int(a) for a, _ in logs[r]] == [2], logs[r]
    assert "injected launch failure" in logs[1][0][1] and "peer rank failed" in logs[0][0][1], logs
    pb = synth.make_problem(5, 2000)
    eng = mvicp.Engine(0)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    log, errors = _fault_sym_rounds(eng, pb, 0, True)
    eng.close()
    assert not errors
    assert not np.array_equal(log[-1][2], log[1][2])      # the rounds after the failure moved the poses
    for r in range(2):
        regime_seq.assert_equal(f"{out}.{r}.npz", log, ("fault_sym", r))


# ---------------------------------------------------------------- a refused evaluation is refused on every rank
GICP = 3             # not an mvicp_metric value: the plane-to-plane objective has calls of its own (mvicp_linearize_gicp / mvicp_optimize_gicp, epsilon 1e-3 here)
REFUSAL_FRAME = 4    # of make_problem(5, .): edges 3->4, 4->3, 4->2 touch it, all owned by rank 1 of 2 (asserted below)


def _refusal_rounds(eng, pb, metric):
    """frame 4 has no normals: evaluate (must be refused), give it normals, evaluate again -> (message of the refusal, blocks after)"""
    import mvicp
    evaluate = (lambda: eng.linearize_gicp(pb["init"], 1e-3, 1)) if metric == GICP else (lambda: eng.linearize_metric(pb["init"], metric, 1))
    eng.correspond(pb["init"], pb["fixed"], 0.05)
    msg = ""
    try:
        evaluate()
    except mvicp.MvicpError as ex:
        msg = str(ex)
    eng.recompute_normals(REFUSAL_FRAME, 10)
    return msg, evaluate()


def _refusal_engine(rank, world, allreduce):
    import mvicp
    from mvicp import synth
    pb = synth.make_problem(5, 1500)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_frames(pb["pts"], [None if k == REFUSAL_FRAME else n for k, n in enumerate(pb["nor"])]); eng.set_graph(pb["src"], pb["dst"])
    if allreduce is not None:
        eng.comm_set_callback(allreduce)
    return eng, pb


def _refusal_worker(rank, world, port, out, metric):
    allreduce = _group(rank, world, port, seconds=60)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    eng, pb = _refusal_engine(rank, world, allreduce)
    msg, blocks = _refusal_rounds(eng, pb, metric)
    eng.close()
    np.save(f"{out}.{rank}.npy", blocks)
    with open(f"{out}.{rank}.log", "w") as f:
        f.write(msg)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("metric", [1, 2, GICP], ids=["PLANE", "SYMMETRIC", "GICP"])
def test_an_evaluation_refused_on_one_rank_is_refused_on_every_rank(tmp_path, metric):
    """check_evaluable looks at the edges a rank owns.  Frame 4 has no normals and only rank 1's edges touch it: rank 1 refuses the evaluation
    (MVICP_ERR_STATE, naming the frame) and enters the collective with the slot poisoned, so rank 0 — which owns nothing to refuse — returns
    MVICP_ERR_COMM from the same call instead of waiting in the all-reduce (the process group's timeout turns such a wait into an exception).
    After mvicp_recompute_normals on that frame on both ranks the next evaluation equals the single process's bytes."""
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    from mvicp import lib as L
    from mvicp import synth
    pb = synth.make_problem(5, 1500)
    own = L.edge_owner([1500] * len(pb["src"]), 2)
    touching = [e for e in range(len(pb["src"])) if REFUSAL_FRAME in (pb["src"][e], pb["dst"][e])]
    assert touching and all(own[e] == 1 for e in touching), (own, touching)
    out = str(tmp_path / "refusal")
    mp.spawn(_refusal_worker, args=(2, _free_port(), out, metric), nprocs=2, join=True)
    msgs = [open(f"{out}.{r}.log").read() for r in range(2)]
    assert "needs normals on frame %d" % REFUSAL_FRAME in msgs[1], msgs
    if metric == GICP:
        assert "gicp needs normals on frame %d" % REFUSAL_FRAME in msgs[1], msgs     # (its own arm of check_evaluable)
    assert "peer rank failed" in msgs[0], msgs
    eng, pb = _refusal_engine(0, 1, None)
    msg, blocks = _refusal_rounds(eng, pb, metric)
    eng.close()
    assert "needs normals on frame %d" % REFUSAL_FRAME in msg, msg
    assert np.any(blocks[touching[0]])
    for r in range(2):
        got = np.load(f"{out}.{r}.npy")
        assert got.tobytes() == blocks.tobytes(), (r, float(np.abs(got - blocks).max()))


# ---------------------------------------------------------------- the plane-to-plane objective, sharded
GICP_ROUNDS = [1, GICP, GICP, 1, GICP]     # per round: PLANE or plane-to-plane.  GICP follows an arming solve, and a plane solve follows GICP


def _gicp_rounds_run(rank, world, allreduce):
    """-> (log, spec.hit): five rounds of search + solve on make_problem(5, 1500)"""
    import mvicp
    from mvicp import synth
    pb = synth.make_problem(5, 1500)
    eng = mvicp.Engine(0, rank=rank, world=world)
    eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
    if allreduce is not None:
        eng.comm_set_callback(allreduce)
    eng.profile(True)
    poses = pb["init"].copy()
    log = []
    for metric in GICP_ROUNDS:
        c, w = eng.correspond(poses, pb["fixed"], 0.05)
        if metric == GICP:
            poses, _ = eng.optimize_gicp(poses, pb["fixed"], mvicp.lib.PARAM_SOPHUS_SE3, 1e-3, True, 50)
        else:
            poses, _ = eng.optimize_metric(poses, pb["fixed"], mvicp.lib.PARAM_SOPHUS_SE3, metric, True, 50)
        log.append((c.copy(), w.tobytes(), poses.copy()))
    hits = eng.profile_get("spec.hit")[1]
    eng.close()
    return log, hits


def _gicp_rounds_worker(rank, world, port, out):
    allreduce = _group(rank, world, port)
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import regime_seq
    log, hits = _gicp_rounds_run(rank, world, allreduce)
    regime_seq.save(f"{out}.{rank}.npz", log)
    np.save(f"{out}.{rank}.hits.npy", np.array([hits]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_gicp_rounds_sharded_match_single_process(tmp_path):
    """mvicp_optimize_gicp on TWO ranks: its evaluations take the exchange branch of evaluate_blocks (upload_rel_sym before the collective, the
    per-rank c->gicp_eps, its own arm of check_evaluable), between plane solves that arm the queued evaluation and consume it.  Five rounds of
    search + solve, objectives PLANE, GICP, GICP, PLANE, GICP at epsilon 1e-3: after EVERY round each rank's counts, weight bits and poses equal
    the single process's bit for bit, and so does the number of evaluations served from the queue."""
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import regime_seq
    out = str(tmp_path / "gicp_rounds")
    mp.spawn(_gicp_rounds_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    log, hits1 = _gicp_rounds_run(0, 1, None)
    assert all(l[0].sum() > 0 for l in log)
    assert not np.array_equal(log[-1][2], log[0][2])      # the later rounds moved the poses
    for r in range(2):
        regime_seq.assert_equal(f"{out}.{r}.npz", log, ("gicp_rounds", r))
        assert np.load(f"{out}.{r}.hits.npy")[0] == hits1, (r, hits1)
