"""-m gpu: mvicp_optimize_gicp through solves that REJECT steps, with two free poses and each parameterization.

The sibling of tests/test_gpu_sym_rejected.py for the plane-to-plane objective at epsilon = 1e-3: after a rejected step the candidate evaluation
has overwritten the blocks buffer (and the extended-precision relative transforms of upload_rel_sym are the candidate's), and the next iteration
solves from the kept H and g.  Problem, starts and the recorded counts: tests/gicpreject.py.  Reference: the host solve (mvicp_lm_solve) over
gicpref.blocks_fp64 on the same lists for all edges; tests/test_gicp_cpu.py checks on the CPU that it rejects as recorded and that no
accept / reject decision is closer than 1e-6 to min_relative_decrease (the smallest margin is 7.8e-5), so the COUNTS must be equal.  Poses
within 1e-8, the suite's per-solve bar (tests/test_gpu_lm_rejected.py)."""
import numpy as np
import pytest

import gicpreject
import lmreject
import mvicp
from test_gpu_lm_rejected import assert_same_solve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(orc):
    pb, corr, w = lmreject.lists_at_init(orc)
    return pb, corr, w


_REFERENCE = {}


def _reference(world, case, max_iterations):
    key = (case, max_iterations)
    if key not in _REFERENCE:
        _REFERENCE[key] = gicpreject.reference_solve(*world, case, max_iterations)
    return _REFERENCE[key]


@pytest.mark.parametrize("max_iterations", [50, 3])
@pytest.mark.parametrize("case", [pytest.param(c, id=gicpreject.case_id(c)) for c in gicpreject.CASES])
def test_gicp_explicit_lists_rejected_steps_match_the_host_solve(world, case, max_iterations):
    angle, robust, param = case
    pb, corr, w = world
    P0, P_ref, sm_ref = _reference(world, case, max_iterations)
    if max_iterations == 50:
        assert (sm_ref["iterations"], sm_ref["successful_steps"]) == gicpreject.MEASURED[case], sm_ref
        if case in gicpreject.REJECTING:
            assert sm_ref["iterations"] - sm_ref["successful_steps"] - 1 >= 2, sm_ref
    else:
        assert sm_ref["termination"] == 0 and sm_ref["iterations"] == 3, sm_ref
    E = mvicp.Engine(0)
    try:
        E.set_frames(pb["pts"], pb["nor"]); E.set_graph(pb["src"], pb["dst"])
        for e in range(len(pb["src"])):
            E.set_correspondences(e, corr[e][0], corr[e][1], w[e])
        E.profile(True)
        hits = E.profile_get("spec.hit")[1]
        P, sm = E.optimize_gicp(P0, pb["fixed"], param, gicpreject.EPS, bool(robust), max_iterations)
        assert sm["evaluations"] == sm["iterations"] + 1, sm   # one device evaluation per iteration, kept or not
        assert_same_solve(P, sm, P_ref, sm_ref, (gicpreject.case_id(case), max_iterations))
        assert np.array_equal(P[0], P0[0])                       # (the fixed pose keeps its values; a zero may come back with the other sign)
        # the engine is as usable after a solve full of rejections as after any other: the same solve again gives the same bytes
        P2, sm2 = E.optimize_gicp(P0, pb["fixed"], param, gicpreject.EPS, bool(robust), max_iterations)
        assert np.array_equal(P, P2) and sm2 == sm, (sm, sm2)
        assert E.profile_get("spec.hit")[1] == hits      # a plane-to-plane evaluation is never served from the queue
    finally:
        E.close()
