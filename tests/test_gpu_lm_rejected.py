"""-m gpu: mvicp_optimize through solves that REJECT steps.

After a rejected step the candidate evaluation has overwritten the blocks buffer and the next iteration solves from the kept H and g with
a smaller radius and the reused diagonal: a path no other GPU test takes (every other solve of the suite accepts all its steps).  The
problems, the starts and the oracle's counts are those of tests/lmreject.py (tests/test_host_lm.py runs them on the CPU and checks there
that no accept / reject decision is closer than 1e-6 to min_relative_decrease; the device blocks agree with the oracle's to 1e-11,
tests/test_gpu_lin_accuracy.py, so no decision can flip and the COUNTS must be equal).  Poses within 1e-8, the per-solve bar of
test_gpu_parity.py::test_random_graphs_costs_and_parameterizations.

Searched cases: mvicp_correspond at the perturbed poses with cutoff 0.5, then mvicp_optimize from the same poses, against the oracle's LM on
the lists mvicp_get_correspondences returns; the solve's first evaluation must be the one the search queued ("spec.hit"), and the solve
must go on to reject.  With the issue's 3.0 rad start the searched lists make the oracle reject nothing (22 / 21 for sophus and quaternion),
so the angle was moved: sophus at 2.0 rad (oracle on the CPU: 18 / 14, 3 rejected, margin 6.0e-2) and quaternion at 1.5 rad (39 / 33, 5
rejected, margin 2.2e-2)."""
import numpy as np
import pytest

import lmreject
import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
SEARCH_CUTOFF = 0.5
# (angle, point_to_plane, robust, param)
SEARCHED = [(2.0, 1, 0, L.PARAM_SOPHUS_SE3), (1.5, 1, 0, L.PARAM_EIGEN_QUATERNION)]


@pytest.fixture(scope="module")
def world(orc):
    pb, corr, w = lmreject.lists_at_init(orc)
    return {"pb": pb, "corr": corr, "w": w}


def assert_same_solve(P, sm, P_ref, sm_ref, tag):
    print(tag, "oracle", sm_ref["iterations"], "/", sm_ref["successful_steps"], "termination", sm_ref["termination"],
          "| GPU", sm["iterations"], "/", sm["successful_steps"], "termination", sm["termination"], "evaluations", sm["evaluations"])
    assert sm["iterations"] == sm_ref["iterations"] and sm["successful_steps"] == sm_ref["successful_steps"], (tag, sm, sm_ref)
    assert sm["termination"] == sm_ref["termination"], (tag, sm, sm_ref)
    worst = 0.0
    for k in range(len(P)):
        dt, dr = synth.pose_diff(P[k], P_ref[k])
        worst = max(worst, dt, dr)
        assert dt < 1e-8 and dr < 1e-8, (tag, k, dt, dr)
    print(tag, "worst pose difference %.2e" % worst)


@pytest.mark.parametrize("max_iterations", [50, 3])
@pytest.mark.parametrize("case", [pytest.param(c, id=lmreject.case_id(c)) for c in lmreject.CASES])
def test_explicit_lists_rejected_steps_match_oracle(orc, world, case, max_iterations):
    angle, plane, robust, param = case
    pb, corr, w = world["pb"], world["corr"], world["w"]
    P0 = lmreject.start_poses(pb, angle)
    prob = orc.make_problem(pb["pts"], pb["nor"], pb["fixed"], pb["src"], pb["dst"], corr, w, param, plane, robust)
    P_ref, sm_ref = orc.optimize(prob, P0, max_iterations)
    if max_iterations == 50:
        assert (sm_ref["iterations"], sm_ref["successful_steps"]) == lmreject.MEASURED[case], sm_ref
        if case in lmreject.REJECTING:
            assert sm_ref["iterations"] - sm_ref["successful_steps"] >= 2, sm_ref
    else:
        assert sm_ref["termination"] == 0 and sm_ref["iterations"] == 3, sm_ref
    E = mvicp.Engine(0)
    try:
        E.set_frames(pb["pts"], pb["nor"]); E.set_graph(pb["src"], pb["dst"])
        for e in range(len(pb["src"])):
            E.set_correspondences(e, corr[e][0], corr[e][1], w[e])
        P, sm = E.optimize(P0, pb["fixed"], param, plane, bool(robust), max_iterations)
        assert sm["evaluations"] == sm["iterations"] + 1, sm   # one device evaluation per iteration, kept or not
        assert_same_solve(P, sm, P_ref, sm_ref, (lmreject.case_id(case), max_iterations))
        # the engine is as usable after a solve full of rejections as after any other: the same solve again gives the same bytes
        P2, sm2 = E.optimize(P0, pb["fixed"], param, plane, bool(robust), max_iterations)
        assert np.array_equal(P, P2) and sm2 == sm, (sm, sm2)
    finally:
        E.close()


@pytest.mark.parametrize("case", [pytest.param(c, id=lmreject.case_id(c)) for c in SEARCHED])
def test_searched_lists_queued_first_evaluation_then_rejected_steps(orc, world, case, monkeypatch, capfd):
    angle, plane, robust, param = case
    pb = world["pb"]
    P0 = lmreject.start_poses(pb, angle)
    E = mvicp.Engine(0)
    try:
        E.set_frames(pb["pts"], pb["nor"]); E.set_graph(pb["src"], pb["dst"])
        # a first round at the unperturbed poses tells the library the solve's flags: the NEXT search queues the first evaluation
        E.correspond(pb["init"], pb["fixed"], SEARCH_CUTOFF)
        E.optimize(pb["init"], pb["fixed"], param, plane, bool(robust), 50)
        E.profile(True); E.profile_reset()
        counts, weights = E.correspond(P0, pb["fixed"], SEARCH_CUTOFF)
        corr = []
        for e in range(len(pb["src"])):
            f, s, _ = E.get_correspondences(e)
            assert len(f) == counts[e]
            corr.append((f, s))
        P, sm = E.optimize(P0, pb["fixed"], param, plane, bool(robust), 50)
        hits = E.profile_get("spec.hit")[1]
    finally:
        E.close()
    assert hits == 1, hits   # the first evaluation was the one the search queued behind its own kernels
    prob = orc.make_problem(pb["pts"], pb["nor"], pb["fixed"], pb["src"], pb["dst"], corr, weights, param, plane, robust)
    P_ref, sm_ref, rd = lmreject.traced_optimize(orc, prob, P0, 50, monkeypatch, capfd)
    margin = lmreject.decision_margin(rd)
    rejected = int((rd <= lmreject.MIN_RELATIVE_DECREASE).sum())
    print(lmreject.case_id(case), "counts", counts.tolist(), "rejected", rejected, "min |relative_decrease - 1e-3| = %.3e" % margin)
    assert rejected >= 1 and sm_ref["iterations"] - sm_ref["successful_steps"] >= 2, (sm_ref, rd)
    assert margin > 1e-6, (margin, rd)
    assert_same_solve(P, sm, P_ref, sm_ref, lmreject.case_id(case))
