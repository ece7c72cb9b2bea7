"""-m gpu: bin/multiview --reject_boundary --reject_mode device, which is how Session::setRejectMasks is tested: the masks go to the search
once and nothing is called per round.  The final poses equal, byte for byte, those of the same loop through Engine.set_reject_mask, without
the copy-back; with it, the frames' lists (--dump_corr) hold no pair on a flagged target and the poses are the same again."""
import os
import re
import subprocess

import numpy as np
import pytest

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
    """the four-view fixture of tests/test_gpu_boundary_driver.py, written to files and read back (both routes see the bytes the files hold)"""
    pb = synth.make_problem(K_VIEWS, N_PTS)
    d = str(tmp_path_factory.mktemp("reject_mask_data"))
    for i in range(K_VIEWS):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([pb["pts"][i], pb["nor"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), pb["init"][i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), pb["gt"][i], fmt="%.17g")
    pts = [np.ascontiguousarray(np.loadtxt(os.path.join(d, f"cloud_{i}.xyz"))[:, :3]) for i in range(K_VIEWS)]
    nor = [np.ascontiguousarray(np.loadtxt(os.path.join(d, f"cloud_{i}.xyz"))[:, 3:]) for i in range(K_VIEWS)]
    init = np.array([np.loadtxt(os.path.join(d, f"pose_{i}.txt")) for i in range(K_VIEWS)])
    return pb, pts, nor, init, d


def _run(d, out, extra):
    os.makedirs(out)
    text = subprocess.check_output([os.path.join(BIN, "multiview"), "--dir", d, "--out", out] + COMMON + extra, universal_newlines=True)
    return text, np.array([np.loadtxt(os.path.join(out, f"pose_{i}.txt")) for i in range(K_VIEWS)])


@pytest.fixture(scope="module")
def engine_route(problem):
    """-> (masks, graph, kept pairs per round, final poses): set_reject_mask once, then the driver's rounds"""
    pb, pts, nor, init, _ = problem
    src, dst = synth.pose_graph_knn(init, 2, skip_fixed0=False)   # (the driver's graph includes the fixed frame's own, inactive edges)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, nor)
        masks = [eng.boundary(i, 30, 0.0, -0.5)["flag"] for i in range(K_VIEWS)]
        for i in range(K_VIEWS):
            eng.set_reject_mask(i, masks[i], L.REJECT_AS_TARGET)
        eng.set_graph(src, dst)
        poses, kept = init.copy(), []
        for _ in range(ROUNDS):
            counts, _ = eng.correspond(poses, pb["fixed"], 0.05)
            kept.append(int(counts.sum()))
            poses, _ = eng.optimize_metric(poses, pb["fixed"], L.PARAM_SOPHUS_SE3, L.METRIC_PLANE, True, 50)
    finally:
        eng.close()
    return masks, (src, dst), kept, poses


def test_device_mode_equals_the_engine_route_without_the_copy_back(problem, engine_route, tmp_path):
    pb, pts, nor, init, d = problem
    masks, _, kept, want = engine_route
    assert all(0 < int(m.sum()) < N_PTS for m in masks) and all(k > 0 for k in kept)
    text, got = _run(d, str(tmp_path / "device"), ["--reject_boundary", "--reject_mode", "device", "--nocopyback"])
    assert [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^boundary: frame (\d+) flagged (\d+) of (\d+)$", text, flags=re.M)] == [
        (i, int(masks[i].sum()), N_PTS) for i in range(K_VIEWS)], text
    assert "dropped" not in text                                  # nothing is called per round
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()


def test_with_the_copy_back_the_frames_hold_no_flagged_target(problem, engine_route, tmp_path):
    pb, pts, nor, init, d = problem
    masks, _, kept, want = engine_route
    dump = str(tmp_path / "corr")
    os.makedirs(dump)
    _, got = _run(d, str(tmp_path / "device_cb"), ["--reject_boundary", "--reject_mode", "device", "--dump_corr", dump])
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    total, files = 0, sorted(f for f in os.listdir(dump) if f.startswith("corr_"))
    assert files
    for name in files:
        with open(os.path.join(dump, name)) as fh:
            head = fh.readline().split()
            j, count = int(head[0]), int(head[2])
            rows = np.loadtxt(fh, ndmin=2) if count else np.zeros((0, 3))   # (the fixed frame's edges are not searched: empty lists)
        assert len(rows) == count
        if count:
            assert not masks[j][rows[:, 1].astype(np.int64)].any(), name
        total += count
    assert total == kept[-1]                                       # the last round's lists, as the search kept them
    # an unknown mode is refused
    r = subprocess.run([os.path.join(BIN, "multiview"), "--dir", d] + COMMON + ["--reject_boundary", "--reject_mode", "gpu"], universal_newlines=True,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and "--reject_mode" in r.stderr
