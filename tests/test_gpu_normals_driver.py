"""-m gpu: bin/multiview --normals_nn 16 --symmetric replaces the recomputeNormals step by Frame::estimateNormals (mvicp_estimate_normals,
the viewpoint at each view's own origin).  On the four-view fixture of tests/test_gpu_init_driver.py, started at the ground truth, it
runs and converges (the criterion of tests/test_gpu_sym_driver.py), and its final poses equal, byte for byte, those of the same
registration driven through Engine with estimate_normals + adopt_normals on every frame.  Its distance from the truth is printed next to
that of the run on the fixture's own normals (--norecomputeNormals), not asserted."""
import os
import subprocess

import numpy as np
import pytest

import initref as ir
import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
K, ROUNDS, CUTOFF, NN = 4, 20, 0.05, 16


def run(d, o, extra):
    trace = os.path.join(str(o), "trace.txt")
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS), "--cutoff", str(CUTOFF),
           "--knn", "3", "--drop_phantom_row", "--quiet", "--symmetric", "--trace", trace] + extra
    subprocess.check_output(cmd, timeout=300)
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    per_round = {}
    for line in open(trace):
        w = line.split()
        if w[0] == "P":
            per_round[(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float64).reshape(4, 4)
    return poses, per_round


def test_driver_with_estimated_normals_converges_and_equals_the_engine_route(tmp_path):
    cl = ir.fixture_clouds()
    d = tmp_path / "data"; a = tmp_path / "est"; b = tmp_path / "own"
    for x in (d, a, b):
        x.mkdir()
    for i in range(K):
        np.savetxt(os.path.join(str(d), f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"pose_{i}.txt"), cl["gt"][i], fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")
    poses_e, tr_e = run(d, a, ["--normals_nn", str(NN)])
    poses_o, tr_o = run(d, b, ["--norecomputeNormals"])
    worst = {}
    for name, poses, tr in (("--normals_nn 16", poses_e, tr_e), ("--norecomputeNormals", poses_o, tr_o)):
        assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
        deg = sp = mdeg = msp = 0.0
        for k in range(1, K):
            e = ir.pose_error(poses[k], cl["gt"][k])
            m = ir.pose_error(tr[(ROUNDS - 1, k)], tr[(ROUNDS - 2, k)])      # what the last round still moved
            deg, sp = max(deg, e[0]), max(sp, e[1] / cl["spacing"])
            mdeg, msp = max(mdeg, m[0]), max(msp, m[1] / cl["spacing"])
        worst[name] = (deg, sp, mdeg, msp)
        print("driver --symmetric %-20s ends %.5f deg, %.5f spacings from the truth; the last round moved %.2e deg, %.2e spacings" % (name, deg, sp, mdeg, msp))
    # converged: the last of the 20 rounds moves no pose by more than a hundredth of a degree or of a spacing (tests/test_gpu_sym_driver.py)
    deg, sp, mdeg, msp = worst["--normals_nn 16"]
    assert mdeg <= 1e-2 and msp <= 1e-2, worst
    assert poses_e.tobytes() != poses_o.tobytes()      # the flag replaces the normals
    # the same registration through Engine
    src, dst = synth.pose_graph_knn(cl["gt"], 3, skip_fixed0=False)
    fixed = np.array([1] + [0] * (K - 1), dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        for i in range(K):
            eng.estimate_normals(i, NN)
            eng.adopt_normals()
        eng.set_graph(src, dst)
        P = cl["gt"].copy()
        for _ in range(ROUNDS):
            eng.correspond(P, fixed, CUTOFF)
            P, _ = eng.optimize_metric(P, fixed, L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
    finally:
        eng.close()
    print("driver against the engine route: largest difference of a pose entry %.3e" % np.abs(poses_e - P).max())
    assert poses_e.tobytes() == np.ascontiguousarray(P).tobytes()
