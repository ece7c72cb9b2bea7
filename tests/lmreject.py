"""Solves that REJECT steps: the problems of tests/test_host_lm.py (CPU) and tests/test_gpu_lm_rejected.py (GPU).  Test infrastructure only.

Problem: synth.make_problem(3, 300, pose_seed=7), lists from the oracle's search at pb["init"] with cutoff 0.05.  Start: pb["init"] with the
rotation of frames 1 and 2 left-multiplied by so3_exp(angle * d_k), d_1 and d_2 two unit directions drawn one after the other (normal(size=3),
normalised) from default_rng(7).  A start 1.5 or 3.0 rad away from the lists' poses makes the first Gauss-Newton models poor: the trust region
shrinks (radius /= 2, 4, 8 ...), the diagonal is reused, H and g stay the kept ones.

Counts of the ORACLE's solve (50 iterations; iterations / successful steps; the stopping iteration is never a successful one, so
iterations - successful_steps - 1 steps were rejected), measured on the CPU; the product's host solve over oracle blocks gives the same:

    angle  cost, loss             quaternion  angle-axis  sophus
    1.5    point-to-plane, plain  15 / 10     15 / 10     7 / 6
    3.0    point-to-plane, plain  23 / 14     37 / 28     10 / 9
    3.0    point-to-plane, robust 21 / 16     41 / 31     18 / 17

The sophus solves reject nothing from these starts (left here as ordinary cases); REJECTING lists the cases that must keep rejecting.
Not a usable case, and left out: the robust loss with the weights scaled by 0.01 at 3.0 rad.  Two of the three parameterizations run into the
50-iteration limit there and the two solvers drift apart to 1e-5 with 40 against 41 successful steps: a chaotic trajectory, not a defect."""
import re

import numpy as np

from mvicp import synth

K, N, POSE_SEED, CUTOFF, DIR_SEED = 3, 300, 7, 0.05, 7
MIN_RELATIVE_DECREASE = 1e-3
# (angle, point_to_plane, robust)
SETTINGS = [(1.5, 1, 0), (3.0, 1, 0), (3.0, 1, 1)]
PARAMS = [0, 1, 2]   # quaternion, angle-axis, sophus
CASES = [(a, p, r, param) for (a, p, r) in SETTINGS for param in PARAMS]
REJECTING = [c for c in CASES if c[3] != 2]
# the oracle's counts above: (iterations, successful_steps); every one of these solves stops on the function tolerance (termination 3)
MEASURED = {(1.5, 1, 0, 0): (15, 10), (1.5, 1, 0, 1): (15, 10), (1.5, 1, 0, 2): (7, 6),
            (3.0, 1, 0, 0): (23, 14), (3.0, 1, 0, 1): (37, 28), (3.0, 1, 0, 2): (10, 9),
            (3.0, 1, 1, 0): (21, 16), (3.0, 1, 1, 1): (41, 31), (3.0, 1, 1, 2): (18, 17)}


def case_id(c):
    return "%.1frad-plane%d-robust%d-param%d" % c


def lists_at_init(orc):
    """-> (pb, corr, w): the problem, per edge (first, second) and the float32 weight of the oracle's search at pb["init"]."""
    pb = synth.make_problem(K, N, pose_seed=POSE_SEED)
    corr, w = [], []
    for s, d in zip(pb["src"], pb["dst"]):
        f, sec, _, wt, _, _ = orc.correspond_edge(pb["pts"][s], pb["init"][s], pb["pts"][d], pb["init"][d], CUTOFF)
        corr.append((f, sec)); w.append(np.float32(wt))
    return pb, corr, w


def start_poses(pb, angle):
    rng = np.random.default_rng(DIR_SEED)
    P = np.array(pb["init"]).copy()
    for k in (1, 2):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        P[k][:3, :3] = synth.so3_exp(angle * d) @ P[k][:3, :3]
    return P


_TRACE = re.compile(r"\[orc lm\] it (\d+) cost (\S+) cand (\S+) .* model_change (\S+)")


def traced_optimize(orc, prob, poses, max_iterations, monkeypatch, capfd):
    """orc.optimize with the oracle's per-iteration log switched on -> (poses, summary, rd): rd = the relative_decrease of every iteration
    that reached the accept / reject decision (an iteration that stops on a tolerance decides nothing)."""
    capfd.readouterr()
    monkeypatch.setenv("ORC_LM_TRACE", "1")
    P, sm = orc.optimize(prob, poses, max_iterations)
    monkeypatch.delenv("ORC_LM_TRACE")
    rows = [(int(m[1]), float(m[2]), float(m[3]), float(m[4])) for m in _TRACE.finditer(capfd.readouterr().err)]
    assert [r[0] for r in rows] == list(range(1, sm["iterations"] + 1)), (rows, sm)   # (no invalid step: every iteration has its line)
    if sm["termination"] in (2, 3):
        rows = rows[:-1]
    rd = np.array([(cost - cand) / mc for _, cost, cand, mc in rows])
    assert int((rd > MIN_RELATIVE_DECREASE).sum()) == sm["successful_steps"], (rd, sm)   # the log and the summary tell the same story
    return P, sm, rd


def decision_margin(rd):
    """smallest distance of a decided relative_decrease from the threshold"""
    return float(np.abs(rd - MIN_RELATIVE_DECREASE).min())
