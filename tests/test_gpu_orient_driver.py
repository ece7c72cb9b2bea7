"""-m gpu: bin/multiview --normals_nn 16 --symmetric --normals_orient mst on the four-view fixture of tests/test_gpu_init_driver.py, started
at the ground truth.  The fixture's views are surface patches in frames whose origin is no sensor, so the viewpoint rule of --normals_nn
leaves the normals of each view on both sides of the surface.  With the flag every view is oriented in itself (Frame::orientNormals) and
the views then agree with each other (Session::orientFrames): the adopted normals of all four views lie on one side of the fixture's, the
run converges (the criterion of tests/test_gpu_normals_driver.py), its final poses equal, byte for byte, those of the same chain driven
through Engine, and it ends closer to the truth, in degrees and in spacings, than the run without the flag, measured in the same test.
Without the flag the driver does what it did: its poses are those of the Engine route of tests/test_gpu_normals_driver.py.  Both figures
are printed next to those of the run on the fixture's own normals."""
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
K, ROUNDS, CUTOFF, NN, ORIENT_NN = 4, 20, 0.05, 16, 10


def run(d, o, extra):
    trace = os.path.join(str(o), "trace.txt")
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS), "--cutoff", str(CUTOFF),
           "--knn", "3", "--drop_phantom_row", "--quiet", "--symmetric", "--trace", trace] + extra
    text = subprocess.check_output(cmd, timeout=300).decode()
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    per_round = {}
    for line in open(trace):
        w = line.split()
        if w[0] == "P":
            per_round[(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float64).reshape(4, 4)
    return poses, per_round, text


def engine_route(cl, orient):
    """estimate -> (orient -> adopt) per frame, (orient_frames,) 20 rounds -> (poses, the adopted normals, what orient_frames returned)"""
    src, dst = synth.pose_graph_knn(cl["gt"], 3, skip_fixed0=False)
    fixed = np.array([1] + [0] * (K - 1), dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        trees = []
        for i in range(K):
            eng.estimate_normals(i, NN)
            if orient:
                trees.append(eng.orient_normals(i, ORIENT_NN, 0.0, 1)["components"])
                eng.adopt_orientation()
            else:
                eng.adopt_normals()
        eng.set_graph(src, dst)
        P = cl["gt"].copy()
        res = mvicp.orient_frames(eng, P, fixed, CUTOFF, 0) if orient else None
        nrm = [eng.get_structure(i, "snor").view(np.float64).reshape(-1, 3)[eng.get_structure(i, "inv").view(np.int32)].copy() for i in range(K)]
        for _ in range(ROUNDS):
            eng.correspond(P, fixed, CUTOFF)
            P, _ = eng.optimize_metric(P, fixed, L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
        return np.ascontiguousarray(P), nrm, res, trees
    finally:
        eng.close()


def test_driver_with_mst_orientation(tmp_path):
    cl = ir.fixture_clouds()
    d = tmp_path / "data"; a = tmp_path / "mst"; b = tmp_path / "view"; c = tmp_path / "own"
    for x in (d, a, b, c):
        x.mkdir()
    for i in range(K):
        np.savetxt(os.path.join(str(d), f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"pose_{i}.txt"), cl["gt"][i], fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")
    poses_m, tr_m, text_m = run(d, a, ["--normals_nn", str(NN), "--normals_orient", "mst", "--orient_nn", str(ORIENT_NN)])
    poses_v, tr_v, text_v = run(d, b, ["--normals_nn", str(NN)])
    poses_o, tr_o, _ = run(d, c, ["--norecomputeNormals"])
    assert "normal orientation" in text_m and "normal orientation" not in text_v
    worst = {}
    for name, poses, tr in (("--normals_orient mst", poses_m, tr_m), ("--normals_nn 16 alone", poses_v, tr_v), ("--norecomputeNormals", poses_o, tr_o)):
        assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
        deg = sp = mdeg = msp = 0.0
        for k in range(1, K):
            e = ir.pose_error(poses[k], cl["gt"][k])
            m = ir.pose_error(tr[(ROUNDS - 1, k)], tr[(ROUNDS - 2, k)])      # what the last round still moved
            deg, sp = max(deg, e[0]), max(sp, e[1] / cl["spacing"])
            mdeg, msp = max(mdeg, m[0]), max(msp, m[1] / cl["spacing"])
        worst[name] = (deg, sp, mdeg, msp)
        print("driver --symmetric %-22s ends %.5f deg, %.5f spacings from the truth; the last round moved %.2e deg, %.2e spacings" % (name, deg, sp, mdeg, msp))
    # the Engine route of the same chain: the same bytes
    P, nrm, res, trees = engine_route(cl, True)
    print("normal orientation through Engine: trees per view", trees, "flip", res["flip"].tolist(), "pos", res["pos"].tolist(), "neg", res["neg"].tolist())
    assert trees == [1, 1, 1, 1] and res["components"] == 1
    for i in range(K):
        assert f"normal orientation: frame {i} trees 1" in text_m
    assert "normal orientation: 1 component(s), flipped " + " ".join(str(int(f)) for f in res["flip"]) in text_m
    print("driver against the engine route: largest difference of a pose entry %.3e" % np.abs(poses_m - P).max())
    assert poses_m.tobytes() == P.tobytes()
    # all four views' adopted normals lie on one common side of the fixture's
    side = np.concatenate([np.sign((nrm[i] * cl["nrm"][i]).sum(1)) for i in range(K)])
    assert (side != 0).all() and int((side != side[0]).sum()) == 0
    # converged: the last of the 20 rounds moves no pose by more than a hundredth of a degree or of a spacing
    deg, sp, mdeg, msp = worst["--normals_orient mst"]
    assert mdeg <= 1e-2 and msp <= 1e-2, worst
    # closer to the truth than the run without the flag, in degrees AND in spacings
    assert deg < worst["--normals_nn 16 alone"][0] and sp < worst["--normals_nn 16 alone"][1], worst
    # without the flag the driver's poses are what they were: the Engine route of tests/test_gpu_normals_driver.py
    Pv, _, _, _ = engine_route(cl, False)
    assert poses_v.tobytes() == Pv.tobytes()
