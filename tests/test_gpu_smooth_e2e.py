"""-m gpu: the registration of tests/test_smooth_cpu.py through the library.  The two clouds of matchref.e2e_clouds with noise of half a
spacing along their normals are registered raw and after Engine.smooth_points(30, degree 2): the smoothed clouds are uploaded, fit_normals(16, 3)
is adopted on both, then 25 rounds of mvicp_correspond + mvicp_optimize_metric with PLANE and with SYMMETRIC.  The smoothed clouds equal
the reference's bytes; the smoothed run ends at most half as far from the truth as the raw one, in degrees and in spacings, as on the CPU."""
import numpy as np
import pytest

import mvicp
import smoothcases as sc
import smoothref
import symref
from mvicp import lib as L
from test_smooth_cpu import assert_smoothing_halves_the_error

pytestmark = pytest.mark.gpu

# tests/test_smooth_cpu.py::test_registration_gains_from_smoothing, (partial, smoothed, symmetric) -> degrees, spacings
CPU = {(False, False, False): (0.5226, 0.8256), (False, False, True): (0.3433, 0.6837), (False, True, False): (0.0752, 0.0851),
       (False, True, True): (0.1092, 0.1480), (True, False, False): (0.7418, 1.4691), (True, False, True): (0.7032, 1.0539),
       (True, True, False): (0.1188, 0.1284), (True, True, True): (0.1163, 0.1519)}


def prepared_engine(clouds, views):
    """an engine holding [dst, src] with fit_normals(FIT_NN, FIT_DEGREE) adopted on both and the edge src -> dst"""
    eng = mvicp.Engine(0)
    eng.set_frames(clouds, None)
    for i in range(2):
        eng.fit_normals(i, sc.FIT_NN, 0.0, views[i], sc.FIT_DEGREE)
        eng.adopt_normals()
    eng.set_graph([1], [0])
    return eng


@pytest.mark.parametrize("partial", [False, True])
def test_registration_gains_from_smoothing_on_the_gpu(partial):
    cl = sc.noisy_pair(partial)
    views = [cl["view_dst"], cl["view_src"]]
    raw = [cl["dst"], cl["src"]]
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(raw, None)
        smooth = [eng.smooth_points(i, sc.SMOOTH_NN, 0.0, views[i], sc.SMOOTH_DEGREE) for i in range(2)]
    finally:
        eng.close()
    for i in range(2):
        want = smoothref.smooth(raw[i], sc.SMOOTH_NN, 0.0, views[i], sc.SMOOTH_DEGREE, 0.0)
        assert want["moved"].all() and smoothref.same(smooth[i], want), i
    got = {}
    for smoothed, clouds in ((False, raw), (True, [s["xyz"] for s in smooth])):
        for metric in (L.METRIC_PLANE, L.METRIC_SYMMETRIC):
            eng = prepared_engine(clouds, views)
            try:
                P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
                for _ in range(25):
                    eng.correspond(P, [1, 0], 3.0 * cl["spacing"])
                    P, _ = eng.optimize_metric(P, [1, 0], L.PARAM_SOPHUS_SE3, metric, True, 50)
            finally:
                eng.close()
            symmetric = metric == L.METRIC_SYMMETRIC
            got[smoothed, symmetric] = symref.distance_to_truth(P[1], cl["truth"], cl["clean_src"], cl["spacing"])
            print("SMOOTH registration (GPU) partial=%s %s, %s: ends %.4f deg, %.4f spacings  (CPU: %.4f, %.4f)" % (
                partial, "smoothed" if smoothed else "raw", "symmetric" if symmetric else "point-to-plane", *got[smoothed, symmetric],
                *CPU[partial, smoothed, symmetric]))
    assert_smoothing_halves_the_error(got)
