"""-m gpu: bin/multiview --symmetric runs the solves on the symmetric objective (MVICP_METRIC_SYMMETRIC) in the parameterisation the other
flags select.  On the four-view fixture of tests/test_gpu_init_driver.py, started at the ground truth, it runs, converges and stays within
three times its measured distance from the truth (and within that test's cap of 1 degree, 1 spacing).  The figures of the symmetric and of the default run are
printed (DESIGN.md section 7.1 quotes them); no improvement is asserted here: the fixture's normals are PCA normals of the sampled clouds."""
import os
import subprocess

import numpy as np
import pytest

import initref as ir

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
K, ROUNDS, CUTOFF = 4, 20, 0.05
# the symmetric run's distance from the truth measured on the MI355X, the largest over frames 1 - 3: 0.02088 degrees and 0.03643 spacings (the
# default run: 0.03601 and 0.09083).  The bound is three times the measured value, in the style of tests/test_gpu_init_driver.py, and below that
# test's cap of 1 degree / 1 spacing in any case.
MEASURED_DEG, MEASURED_SPACINGS = 0.02088, 0.03643


def run(d, o, extra):
    trace = os.path.join(str(o), "trace.txt")
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS), "--cutoff", str(CUTOFF),
           "--knn", "3", "--norecomputeNormals", "--drop_phantom_row", "--quiet", "--trace", trace] + extra
    out = subprocess.check_output(cmd, timeout=300).decode().splitlines()
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    per_round = {}
    for line in open(trace):
        w = line.split()
        if w[0] == "P":
            per_round[(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float64).reshape(4, 4)
    return out, poses, per_round


def test_symmetric_driver_run_converges_near_the_truth(tmp_path):
    cl = ir.fixture_clouds()
    d = tmp_path / "data"; a = tmp_path / "sym"; b = tmp_path / "plane"
    for x in (d, a, b):
        x.mkdir()
    for i in range(K):
        np.savetxt(os.path.join(str(d), f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"pose_{i}.txt"), cl["gt"][i], fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")
    _, poses_s, tr_s = run(d, a, ["--symmetric"])
    _, poses_p, tr_p = run(d, b, [])
    worst = {}
    for name, poses, tr in (("symmetric", poses_s, tr_s), ("point-to-plane", poses_p, tr_p)):
        assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
        deg = sp = mdeg = msp = 0.0
        for k in range(1, K):
            e = ir.pose_error(poses[k], cl["gt"][k])
            m = ir.pose_error(tr[(ROUNDS - 1, k)], tr[(ROUNDS - 2, k)])      # what the last round still moved
            deg, sp = max(deg, e[0]), max(sp, e[1] / cl["spacing"])
            mdeg, msp = max(mdeg, m[0]), max(msp, m[1] / cl["spacing"])
        worst[name] = (deg, sp, mdeg, msp)
        print("driver %-14s ends %.5f deg, %.5f spacings from the truth; the last round moved %.2e deg, %.2e spacings" % (name, deg, sp, mdeg, msp))
    deg, sp, mdeg, msp = worst["symmetric"]
    bound_deg, bound_sp = min(3.0 * MEASURED_DEG, 1.0), min(3.0 * MEASURED_SPACINGS, 1.0)
    assert deg <= bound_deg and sp <= bound_sp, worst
    # converged: the last of the 20 rounds moves no pose by more than a hundredth of a degree or of a spacing (the level the two objectives differ at is ten times that)
    assert mdeg <= 1e-2 and msp <= 1e-2, worst
    assert poses_s.tobytes() != poses_p.tobytes()      # the flag selects another objective
