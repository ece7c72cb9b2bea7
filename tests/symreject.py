"""SYMMETRIC solves that REJECT steps: tests/lmreject.py's problem for mvicp_optimize_metric(MVICP_METRIC_SYMMETRIC) — the cases of
tests/test_sym_cpu.py (CPU) and tests/test_gpu_sym_rejected.py (GPU).  Test infrastructure only.

Problem and starts: lmreject's (synth.make_problem(3, 300, pose_seed=7), two free poses, the oracle's lists at pb["init"] with cutoff 0.05,
start_poses(angle)).  Reference: the product's host solve (mvicp_lm_solve, mvicp.lib.lm_solve_host) over symref.blocks_fp64 on the same lists
for all edges — the construction of tests/test_gpu_sym_api.py::test_symmetric_solve_equals_the_host_solve_over_the_fp64_rows; the oracle has
no symmetric rows.  Its accept / reject decisions are read from the solve's own trace (MVICP_LM_TRACE, host/lm.cpp).

Counts of that reference solve, 50 iterations (iterations / successful steps; the stopping iteration is never a successful one, so
iterations - successful_steps - 1 steps were rejected), and the smallest |relative_decrease - min_relative_decrease| over the decisions of
the solve, measured on the CPU; every solve stops on the function tolerance (termination 3):

    angle  loss    quaternion            angle-axis            sophus
    1.5    plain   18 / 13  (7.0e-2)     19 / 13  (8.2e-2)     8 / 7    (1.0)
    1.5    robust  16 / 12  (5.3e-2)     17 / 12  (6.3e-2)     10 / 9   (1.2)
    3.0    plain   25 / 18  (3.3e-1)     21 / 16  (5.2e-1)     14 / 13  (9.9e-1)
    3.0    robust  23 / 18  (2.0e-1)     20 / 17  (1.9e-1)     18 / 17  (1.5)

The sophus solves reject nothing from 1.5 and 3.0 rad, as with the plane objective — and from no other start tried: 0.5, 0.8, 1.0, 1.2, 1.3,
1.4, 1.6, 1.7, 1.8, 2.0, 2.2, 2.5, 2.6, 2.7, 2.8, 2.9, 3.1 rad, plain and robust, each ends with iterations = successful_steps + 1.  They are
left here as ordinary cases at the two angles; REJECTING lists the cases that must keep rejecting (at least two rejected steps, every
decision more than 1e-6 from the threshold)."""
import re

import numpy as np

import lmreject
import symref
from mvicp import lib as L

MIN_RELATIVE_DECREASE = lmreject.MIN_RELATIVE_DECREASE
# (angle, robust, param)
CASES = [(a, r, p) for a in (1.5, 3.0) for r in (0, 1) for p in (L.PARAM_EIGEN_QUATERNION, L.PARAM_ANGLE_AXIS, L.PARAM_SOPHUS_SE3)]
REJECTING = [c for c in CASES if c[2] != L.PARAM_SOPHUS_SE3]
# the reference's counts: (iterations, successful_steps)
MEASURED = {(1.5, 0, 0): (18, 13), (1.5, 0, 1): (19, 13), (1.5, 0, 2): (8, 7),
            (1.5, 1, 0): (16, 12), (1.5, 1, 1): (17, 12), (1.5, 1, 2): (10, 9),
            (3.0, 0, 0): (25, 18), (3.0, 0, 1): (21, 16), (3.0, 0, 2): (14, 13),
            (3.0, 1, 0): (23, 18), (3.0, 1, 1): (20, 17), (3.0, 1, 2): (18, 17)}
# smallest |relative_decrease - 1e-3| of the reference solve, rounded DOWN to two digits (the CPU test asserts at least this much, and > 1e-6)
MEASURED_MARGIN = {(1.5, 0, 0): 7.0e-2, (1.5, 0, 1): 8.2e-2, (1.5, 0, 2): 9.9e-1,
                   (1.5, 1, 0): 5.3e-2, (1.5, 1, 1): 6.2e-2, (1.5, 1, 2): 1.2,
                   (3.0, 0, 0): 3.2e-1, (3.0, 0, 1): 5.1e-1, (3.0, 0, 2): 9.9e-1,
                   (3.0, 1, 0): 1.9e-1, (3.0, 1, 1): 1.9e-1, (3.0, 1, 2): 1.4}


def case_id(c):
    return "%.1frad-robust%d-param%d" % c


def evaluator(pb, corr, w, robust):
    """poses -> E x 91: symref.blocks_fp64 of every edge on its list"""
    def ev(poses):
        out = np.zeros((len(pb["src"]), L.EDGE_BLOCK))
        for e, (s, d) in enumerate(zip(pb["src"], pb["dst"])):
            f, sec = corr[e]
            out[e] = symref.blocks_fp64(pb["pts"][s][f], pb["pts"][d][sec], pb["nor"][d][sec], pb["nor"][s][f], poses[s], poses[d], w[e], robust)
        return out
    return ev


def reference_solve(pb, corr, w, case, max_iterations):
    angle, robust, param = case
    P0 = lmreject.start_poses(pb, angle)
    P, sm = L.lm_solve_host(len(pb["pts"]), pb["src"], pb["dst"], P0, pb["fixed"], param, evaluator(pb, corr, w, robust), max_iterations)
    return P0, P, sm


_TRACE = re.compile(r"\[mvicp lm\] it (\d+) cost (\S+) cand (\S+) .* model_change (\S+)")


def traced_reference_solve(pb, corr, w, case, max_iterations, monkeypatch, capfd):
    """reference_solve with the solve's per-iteration log on -> (P0, P, summary, rd): rd = the relative_decrease of every iteration that
    reached the accept / reject decision (lmreject.traced_optimize's part for the host solve)"""
    capfd.readouterr()
    monkeypatch.setenv("MVICP_LM_TRACE", "1")
    P0, P, sm = reference_solve(pb, corr, w, case, max_iterations)
    monkeypatch.delenv("MVICP_LM_TRACE")
    rows = [(int(m[1]), float(m[2]), float(m[3]), float(m[4])) for m in _TRACE.finditer(capfd.readouterr().err)]
    assert [r[0] for r in rows] == list(range(1, sm["iterations"] + 1)), (rows, sm)   # (no invalid step: every iteration has its line)
    if sm["termination"] in (2, 3):
        rows = rows[:-1]
    rd = np.array([(cost - cand) / mc for _, cost, cand, mc in rows])
    assert int((rd > MIN_RELATIVE_DECREASE).sum()) == sm["successful_steps"], (rd, sm)   # the log and the summary tell the same story
    return P0, P, sm, rd
