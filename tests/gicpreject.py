"""Plane-to-plane solves that REJECT steps: tests/lmreject.py's problem for mvicp_optimize_gicp at epsilon = 1e-3 — the cases of
tests/test_gicp_cpu.py (CPU) and tests/test_gpu_gicp_rejected.py (GPU).  The sibling of tests/symreject.py.  Test infrastructure only.

Problem and starts: lmreject's (synth.make_problem(3, 300, pose_seed=7), two free poses, the oracle's lists at pb["init"] with cutoff 0.05,
start_poses(angle)).  Reference: the product's host solve (mvicp_lm_solve, mvicp.lib.lm_solve_host) over gicpref.blocks_fp64 on the same lists
for all edges.  Its accept / reject decisions are read from the solve's own trace (MVICP_LM_TRACE, host/lm.cpp).

Counts of that reference solve, 50 iterations (iterations / successful steps; the stopping iteration is never a successful one, so
iterations - successful_steps - 1 steps were rejected), and the smallest |relative_decrease - min_relative_decrease| over the decisions of
the solve, measured on the CPU; every solve stops on the function tolerance (termination 3) except 3.0 rad / robust / angle-axis, which is
still taking steps at the 50-iteration limit (termination 0, AT_LIMIT):

    angle  loss    quaternion            angle-axis            sophus
    1.5    plain   23 / 18  (7.8e-5)     25 / 19  (3.4e-1)     7 / 6    (7.3e-1)
    1.5    robust  22 / 17  (7.6e-2)     24 / 18  (2.6e-1)     8 / 7    (7.5e-1)
    3.0    plain   27 / 20  (9.1e-2)     47 / 36  (1.0e-2)     10 / 9   (9.3e-1)
    3.0    robust  12 / 11  (8.5e-2)     50 / 43  (1.2e-1)     11 / 10  (7.6e-1)

The sophus solves reject nothing, as with the other objectives, and neither does the robust quaternion solve from 3.0 rad; they are left here as
ordinary cases.  REJECTING lists the cases that must keep rejecting (at least two rejected steps, every decision more than 1e-6 from the
threshold): seven, both losses and both the quaternion and the angle-axis parameterization among them, so no further start was needed (1.0, 2.0
and 2.5 rad were measured too: every quaternion and angle-axis solve from them rejects 3 to 6 steps)."""
import numpy as np

import gicpref
import lmreject
import symreject
from mvicp import lib as L

EPS = 1e-3
MIN_RELATIVE_DECREASE = lmreject.MIN_RELATIVE_DECREASE
ANGLES = (1.5, 3.0)
# (angle, robust, param)
CASES = [(a, r, p) for a in ANGLES for r in (0, 1) for p in (L.PARAM_EIGEN_QUATERNION, L.PARAM_ANGLE_AXIS, L.PARAM_SOPHUS_SE3)]
# the reference's counts: (iterations, successful_steps)
MEASURED = {(1.5, 0, 0): (23, 18), (1.5, 0, 1): (25, 19), (1.5, 0, 2): (7, 6),
            (1.5, 1, 0): (22, 17), (1.5, 1, 1): (24, 18), (1.5, 1, 2): (8, 7),
            (3.0, 0, 0): (27, 20), (3.0, 0, 1): (47, 36), (3.0, 0, 2): (10, 9),
            (3.0, 1, 0): (12, 11), (3.0, 1, 1): (50, 43), (3.0, 1, 2): (11, 10)}
# every solve stops on the function tolerance (termination 3) but this one, which is still moving at the 50-iteration limit (termination 0)
AT_LIMIT = [(3.0, 1, 1)]
# smallest |relative_decrease - 1e-3| of the reference solve, rounded DOWN to two digits (the CPU test asserts at least this much, and > 1e-6)
MEASURED_MARGIN = {(1.5, 0, 0): 7.8e-5, (1.5, 0, 1): 3.4e-1, (1.5, 0, 2): 7.3e-1,
                   (1.5, 1, 0): 7.6e-2, (1.5, 1, 1): 2.6e-1, (1.5, 1, 2): 7.5e-1,
                   (3.0, 0, 0): 9.1e-2, (3.0, 0, 1): 1.0e-2, (3.0, 0, 2): 9.3e-1,
                   (3.0, 1, 0): 8.5e-2, (3.0, 1, 1): 1.2e-1, (3.0, 1, 2): 7.6e-1}
REJECTING = [c for c in CASES if c in MEASURED and MEASURED[c][0] - MEASURED[c][1] - 1 >= 2]

case_id = symreject.case_id


def evaluator(pb, corr, w, robust):
    """poses -> E x 91: gicpref.blocks_fp64 of every edge on its list"""
    def ev(poses):
        out = np.zeros((len(pb["src"]), L.EDGE_BLOCK))
        for e, (s, d) in enumerate(zip(pb["src"], pb["dst"])):
            f, sec = corr[e]
            out[e] = gicpref.blocks_fp64(pb["pts"][s][f], pb["pts"][d][sec], pb["nor"][d][sec], pb["nor"][s][f], poses[s], poses[d], w[e], EPS, robust)
        return out
    return ev


def reference_solve(pb, corr, w, case, max_iterations):
    angle, robust, param = case
    P0 = lmreject.start_poses(pb, angle)
    P, sm = L.lm_solve_host(len(pb["pts"]), pb["src"], pb["dst"], P0, pb["fixed"], param, evaluator(pb, corr, w, robust), max_iterations)
    return P0, P, sm


def traced_reference_solve(pb, corr, w, case, max_iterations, monkeypatch, capfd):
    """reference_solve with the solve's per-iteration log on -> (P0, P, summary, rd): rd = the relative_decrease of every iteration that
    reached the accept / reject decision (symreject.traced_reference_solve for this evaluator)"""
    capfd.readouterr()
    monkeypatch.setenv("MVICP_LM_TRACE", "1")
    P0, P, sm = reference_solve(pb, corr, w, case, max_iterations)
    monkeypatch.delenv("MVICP_LM_TRACE")
    rows = [(int(m[1]), float(m[2]), float(m[3]), float(m[4])) for m in symreject._TRACE.finditer(capfd.readouterr().err)]
    assert [r[0] for r in rows] == list(range(1, sm["iterations"] + 1)), (rows, sm)   # (no invalid step: every iteration has its line)
    if sm["termination"] in (2, 3):
        rows = rows[:-1]
    rd = np.array([(cost - cand) / mc for _, cost, cand, mc in rows])
    assert int((rd > MIN_RELATIVE_DECREASE).sum()) == sm["successful_steps"], (rd, sm)   # the log and the summary tell the same story
    return P0, P, sm, rd
