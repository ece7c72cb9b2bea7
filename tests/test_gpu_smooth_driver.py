"""-m gpu: bin/multiview --smooth_nn 30 --smooth_iters 2 on the four-view fixture of tests/test_gpu_fit_driver.py with noise of half a spacing
along the normals, in that test's chain (--normals_nn 16 --normals_fit 3 --symmetric --normals_orient mst, started at the ground truth).  The
run's final poses equal, byte for byte, those of the same chain driven through Engine (two passes of smooth_points per view, then that
test's route), and differ from the run without the flag.  The distances from the truth are printed, not asserted.  A second, short run
keeps the normals the smoothing hands over (--norecomputeNormals): Frame::smoothPoints turned them to the side of the frame's own.  The
flags' refusals."""
import os
import subprocess

import numpy as np
import pytest

import initref as ir
import mvicp
import smoothcases as sc
from mvicp import lib as L
from mvicp import synth
from test_gpu_fit_driver import DEGREE, engine_route, write_fixture
from test_gpu_orient_driver import BIN, CUTOFF, K, NN, ORIENT_NN, run

pytestmark = pytest.mark.gpu
PASSES = 2


def engine_smoothing(cl, passes):
    """`passes` passes of smooth_points per view, each uploaded in place of the view, the normals turned to the side of the view's own
    -> (clouds, normals, [(moved, largest |shift|) of the last pass])"""
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        xyz, nrm, last = [], [], []
        for i in range(K):
            own = cl["nrm"][i]
            for _ in range(passes):
                s = eng.smooth_points(i, sc.SMOOTH_NN, 0.0, None, sc.SMOOTH_DEGREE)
                g = s["nrm"]
                dot = (g[:, 0] * own[:, 0] + g[:, 1] * own[:, 1]) + g[:, 2] * own[:, 2]
                own = np.ascontiguousarray(np.where((dot < 0)[:, None], -g, g))
                eng.set_frame(i, s["xyz"], own)
            xyz.append(s["xyz"]); nrm.append(own); last.append((int(s["moved"].sum()), float(np.abs(s["shift"]).max())))
        return xyz, nrm, last
    finally:
        eng.close()


def worst_error(poses, cl):
    deg = sp = 0.0
    for k in range(1, K):
        e = ir.pose_error(poses[k], cl["gt"][k])
        deg, sp = max(deg, e[0]), max(sp, e[1] / cl["spacing"])
    return deg, sp


def test_driver_with_smoothing(tmp_path):
    cl = sc.noisy_fixture()
    d = tmp_path / "data"; a = tmp_path / "smooth"; b = tmp_path / "raw"
    for x in (d, a, b):
        x.mkdir()
    write_fixture(cl, d)
    common = ["--normals_nn", str(NN), "--normals_fit", str(DEGREE), "--normals_orient", "mst", "--orient_nn", str(ORIENT_NN)]
    poses_s, _, text = run(d, a, common + ["--smooth_nn", str(sc.SMOOTH_NN), "--smooth_iters", str(PASSES)])
    poses_r, _, text_r = run(d, b, common)
    assert "smooth:" not in text_r
    for name, poses in (("--smooth_nn 30 --smooth_iters 2", poses_s), ("without --smooth_nn", poses_r)):
        assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
        print("driver --symmetric --normals_fit 3 %-32s ends %.5f deg, %.5f spacings from the truth" % ((name,) + worst_error(poses, cl)))
    xyz, nrm, last = engine_smoothing(cl, PASSES)
    for i, (moved, largest) in enumerate(last):
        assert "smooth: frame %d moved %d of %d, largest |shift| %.17g" % (i, moved, len(xyz[i]), largest) in text, (i, text)
    P, _ = engine_route(dict(cl, xyz=xyz, nrm=nrm))
    print("driver against the engine route: largest difference of a pose entry %.3e" % np.abs(poses_s - P).max())
    assert poses_s.tobytes() == P.tobytes()
    assert poses_s.tobytes() != poses_r.tobytes()      # the flag reached the clouds


def test_the_smoothed_frame_keeps_its_orientation(tmp_path):
    """--norecomputeNormals: the normals the registration runs on are the ones Frame::smoothPoints left -- the call's fitted normals, each on
    the side of the frame's own.  5 rounds; the same bytes as the Engine route with the rule applied in numpy."""
    cl = sc.noisy_fixture()
    d = tmp_path / "data"; a = tmp_path / "out"
    d.mkdir(); a.mkdir()
    write_fixture(cl, d)
    trace = os.path.join(str(a), "trace.txt")
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(a), "--step", "1", "--limit", "40", "--rounds", "5", "--cutoff", str(CUTOFF), "--knn", "3",
           "--drop_phantom_row", "--quiet", "--symmetric", "--trace", trace, "--norecomputeNormals", "--smooth_nn", str(sc.SMOOTH_NN), "--smooth_degree", "3",
           "--smooth_max_shift", str(cl["spacing"])]
    text = subprocess.check_output(cmd, timeout=300).decode()
    poses = np.array([np.loadtxt(os.path.join(str(a), f"pose_{i}.txt")) for i in range(K)])
    src, dst = synth.pose_graph_knn(cl["gt"], 3, skip_fixed0=False)
    fixed = np.array([1] + [0] * (K - 1), dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        xyz, nrm = [], []
        for i in range(K):
            s = eng.smooth_points(i, sc.SMOOTH_NN, 0.0, None, 3, cl["spacing"])
            g, own = s["nrm"], cl["nrm"][i]
            dot = (g[:, 0] * own[:, 0] + g[:, 1] * own[:, 1]) + g[:, 2] * own[:, 2]
            assert (dot < 0).sum() > 10 and (dot > 0).sum() > 10 and 30 < s["moved"].sum() < len(own) - 30      # both signs occur, and the limit bites
            assert "smooth: frame %d moved %d of %d, largest |shift| %.17g" % (i, s["moved"].sum(), len(own), np.abs(s["shift"]).max()) in text
            xyz.append(s["xyz"]); nrm.append(np.ascontiguousarray(np.where((dot < 0)[:, None], -g, g)))
        eng.set_frames(xyz, nrm)
        eng.set_graph(src, dst)
        P = cl["gt"].copy()
        for _ in range(5):
            eng.correspond(P, fixed, CUTOFF)
            P, _ = eng.optimize_metric(P, fixed, L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
    finally:
        eng.close()
    assert poses.tobytes() == np.ascontiguousarray(P).tobytes()


@pytest.mark.parametrize("extra,flag", [(["--smooth_nn", "30", "--smooth_degree", "4"], b"--smooth_degree"), (["--smooth_nn", "30", "--smooth_degree", "1"], b"--smooth_degree"),
                                        (["--smooth_nn", "30", "--smooth_iters", "0"], b"--smooth_iters"), (["--smooth_iters", "2"], b"--smooth_iters"),
                                        (["--smooth_radius", "0.1"], b"--smooth_radius"), (["--smooth_degree", "3"], b"--smooth_degree"),
                                        (["--smooth_max_shift", "0.01"], b"--smooth_max_shift")])
def test_the_flags_are_refused(tmp_path, extra, flag):
    r = subprocess.run([os.path.join(BIN, "multiview"), "--dir", str(tmp_path), "--quiet"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and flag in r.stderr
