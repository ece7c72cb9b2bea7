"""-m gpu: bin/multiview --normals_nn 16 --normals_fit 3 --symmetric --normals_orient mst on the four-view fixture of
tests/test_gpu_orient_driver.py, started at the ground truth.  The run's final poses equal, byte for byte, those of the same chain driven
through Engine (fit_normals in place of estimate_normals), and it converges by the criterion of that test.  Its distance from the truth is
printed next to the run without --normals_fit; that comparison is a measurement, not an assertion.  The flag is refused without
--normals_nn and for a degree other than 2 or 3."""
import os
import subprocess

import numpy as np
import pytest

import initref as ir
import mvicp
from mvicp import lib as L
from mvicp import synth
from test_gpu_orient_driver import BIN, CUTOFF, K, NN, ORIENT_NN, ROUNDS, run

pytestmark = pytest.mark.gpu
DEGREE = 3


def engine_route(cl):
    """fit -> orient -> adopt per frame, orient_frames, 20 rounds -> poses"""
    src, dst = synth.pose_graph_knn(cl["gt"], 3, skip_fixed0=False)
    fixed = np.array([1] + [0] * (K - 1), dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        fell_back = []
        for i in range(K):
            fell_back.append(int((eng.fit_normals(i, NN, 0.0, None, DEGREE)["fitted"] == 0).sum()))
            eng.orient_normals(i, ORIENT_NN, 0.0, 1)
            eng.adopt_orientation()
        eng.set_graph(src, dst)
        P = cl["gt"].copy()
        mvicp.orient_frames(eng, P, fixed, CUTOFF, 0)
        for _ in range(ROUNDS):
            eng.correspond(P, fixed, CUTOFF)
            P, _ = eng.optimize_metric(P, fixed, L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
        return np.ascontiguousarray(P), fell_back
    finally:
        eng.close()


def write_fixture(cl, d):
    for i in range(K):
        np.savetxt(os.path.join(str(d), f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"pose_{i}.txt"), cl["gt"][i], fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")


def test_driver_with_fitted_normals(tmp_path):
    cl = ir.fixture_clouds()
    d = tmp_path / "data"; a = tmp_path / "fit"; b = tmp_path / "pca"
    for x in (d, a, b):
        x.mkdir()
    write_fixture(cl, d)
    common = ["--normals_nn", str(NN), "--normals_orient", "mst", "--orient_nn", str(ORIENT_NN)]
    poses_f, tr_f, _ = run(d, a, common + ["--normals_fit", str(DEGREE)])
    poses_p, tr_p, _ = run(d, b, common)
    worst = {}
    for name, poses, tr in (("--normals_fit 3", poses_f, tr_f), ("without --normals_fit", poses_p, tr_p)):
        assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
        deg = sp = mdeg = msp = 0.0
        for k in range(1, K):
            e = ir.pose_error(poses[k], cl["gt"][k])
            m = ir.pose_error(tr[(ROUNDS - 1, k)], tr[(ROUNDS - 2, k)])      # what the last round still moved
            deg, sp = max(deg, e[0]), max(sp, e[1] / cl["spacing"])
            mdeg, msp = max(mdeg, m[0]), max(msp, m[1] / cl["spacing"])
        worst[name] = (deg, sp, mdeg, msp)
        print("driver --symmetric --normals_orient mst %-22s ends %.5f deg, %.5f spacings from the truth; the last round moved %.2e deg, %.2e spacings" % (
            name, deg, sp, mdeg, msp))
    P, fell_back = engine_route(cl)
    print("rows that kept the PCA normal, per view:", fell_back)
    print("driver against the engine route: largest difference of a pose entry %.3e" % np.abs(poses_f - P).max())
    assert poses_f.tobytes() == P.tobytes()
    assert poses_f.tobytes() != poses_p.tobytes()      # the flag reached the normals
    # converged: the last of the 20 rounds moves no pose by more than a hundredth of a degree or of a spacing
    deg, sp, mdeg, msp = worst["--normals_fit 3"]
    assert mdeg <= 1e-2 and msp <= 1e-2, worst


@pytest.mark.parametrize("extra", [["--normals_fit", "3"], ["--normals_nn", "16", "--normals_fit", "4"], ["--normals_nn", "16", "--normals_fit", "1"]])
def test_the_flag_is_refused(tmp_path, extra):
    r = subprocess.run([os.path.join(BIN, "multiview"), "--dir", str(tmp_path), "--quiet"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and b"--normals_fit" in r.stderr
