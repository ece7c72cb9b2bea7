"""-m gpu: the boundary flags of the headless driver (mv-lm-icp_amd/bin/multiview --reject_boundary / --boundary_nn / --boundary_radius /
--boundary_cos), which is how Frame::boundaryPoints and Session::rejectBoundary are tested: the lines it prints are the reference's and the
Engine route's numbers, and its final poses equal, byte for byte, those of the same loop through Engine.reject_correspondences."""
import os
import re
import subprocess

import numpy as np
import pytest

import boundref as br
import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
K_VIEWS, N_PTS, ROUNDS = 4, 3000, 6
COMMON = ["--step", "1", "--limit", "40", "--quiet", "--norecomputeNormals", "--drop_phantom_row", "--rounds", str(ROUNDS)]


@pytest.fixture(scope="module")
def problem(tmp_path_factory):
    pb = synth.make_problem(K_VIEWS, N_PTS)
    d = str(tmp_path_factory.mktemp("boundary_data"))
    for i in range(K_VIEWS):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([pb["pts"][i], pb["nor"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), pb["init"][i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), pb["gt"][i], fmt="%.17g")
    # the driver reads the files: the Engine route must see the bytes the files hold
    pts = [np.ascontiguousarray(np.loadtxt(os.path.join(d, f"cloud_{i}.xyz"))[:, :3]) for i in range(K_VIEWS)]
    nor = [np.ascontiguousarray(np.loadtxt(os.path.join(d, f"cloud_{i}.xyz"))[:, 3:]) for i in range(K_VIEWS)]
    init = np.array([np.loadtxt(os.path.join(d, f"pose_{i}.txt")) for i in range(K_VIEWS)])
    return pb, pts, nor, init, d


def _run(d, out, extra):
    os.makedirs(out)
    text = subprocess.check_output([os.path.join(BIN, "multiview"), "--dir", d, "--out", out] + COMMON + extra, universal_newlines=True)
    poses = np.array([np.loadtxt(os.path.join(out, f"pose_{i}.txt")) for i in range(K_VIEWS)])
    return text, poses


def _engine_route(pts, nor, init, fixed, args, param, metric):
    """-> (flagged per frame, dropped per round, final poses) of the driver's loop through the Python binding"""
    src, dst = synth.pose_graph_knn(init, 2, skip_fixed0=False)   # (the driver's graph includes the fixed frame's own, inactive edges)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, nor)
        masks = [eng.boundary(i, *args)["flag"] for i in range(K_VIEWS)]
        eng.set_graph(src, dst)
        poses, dropped = init.copy(), []
        for _ in range(ROUNDS):
            eng.correspond(poses, fixed, 0.05)
            dropped.append(int(eng.reject_correspondences(masks).sum()))
            poses, _ = eng.optimize_metric(poses, fixed, param, metric, True, 50)
    finally:
        eng.close()
    return masks, dropped, poses


@pytest.mark.parametrize("flags,args,metric", [([], (30, 0.0, -0.5), L.METRIC_PLANE),
                                                (["--boundary_nn", "16", "--boundary_cos", "0.0", "--symmetric"], (16, 0.0, 0.0), L.METRIC_SYMMETRIC)])
def test_driver_equals_the_engine_route(problem, tmp_path, flags, args, metric):
    pb, pts, nor, init, d = problem
    masks, dropped, want = _engine_route(pts, nor, init, pb["fixed"], args, L.PARAM_SOPHUS_SE3, metric)
    for i in range(K_VIEWS):   # the masks are the reference's, with flagged and unflagged points in every view
        ref = br.boundary(pts[i], nor[i], *args)
        assert masks[i].tobytes() == ref["flag"].tobytes() and 0 < ref["boundary"] < N_PTS
    assert all(x > 0 for x in dropped)
    plain_text, plain = _run(d, str(tmp_path / "plain"), [f for f in flags if f == "--symmetric"])
    assert "boundary:" not in plain_text                                              # default off
    text, got = _run(d, str(tmp_path / "reject"), ["--reject_boundary"] + flags)
    assert [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^boundary: frame (\d+) flagged (\d+) of (\d+)$", text, flags=re.M)] == [
        (i, int(masks[i].sum()), N_PTS) for i in range(K_VIEWS)], text
    assert [(int(a), int(b)) for a, b in re.findall(r"^boundary: round (\d+) dropped (\d+) pairs$", text, flags=re.M)] == list(enumerate(dropped)), (text, dropped)
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    # distance to the ground truth with and without the flag: printed, not asserted (the four views overlap almost fully)
    err = lambda P: np.sum([synth.pose_diff(P[i], pb["gt"][i]) for i in range(K_VIEWS)], axis=0)
    print("pose_diff sums (dt, dr): without the flag", err(plain), "with", err(got))


def test_what_the_driver_refuses(problem):
    """(The third refusal, a frame without normals after the pre-processing, cannot be reached from files: the loader gives every point a
    normal.  Frame::boundaryPoints refuses such a frame itself.)"""
    d = problem[4]
    run = lambda extra: subprocess.run([os.path.join(BIN, "multiview"), "--dir", d] + COMMON + extra, universal_newlines=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for bad in ("1", "-1", "1.5"):
        r = run(["--reject_boundary", "--boundary_cos=" + bad])
        assert r.returncode == 1 and "--boundary_cos" in r.stderr, (bad, r.stderr)
    r = run(["--reject_boundary", "--nocopyback"])
    assert r.returncode == 1 and "copyback" in r.stderr
