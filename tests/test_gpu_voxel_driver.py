"""-m gpu: the voxel-grid flags of the headless driver (mv-lm-icp_amd/bin/multiview): the fused model it writes is mvicp_voxel_grid at the
poses it writes, byte for byte, and a coarse-to-fine run equals the same sequence of engine calls."""
import os
import subprocess

import numpy as np
import pytest

import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
COMMON = ["--step", "1", "--limit", "40", "--quiet", "--norecomputeNormals", "--drop_phantom_row"]


def write_dataset(d, pb):
    """The reference's on-disk formats, as tests/test_gpu_drivers.py writes them (17 digits: every double survives the round trip)."""
    for i, (p, n) in enumerate(zip(pb["pts"], pb["nor"])):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([p, n]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), pb["init"][i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), pb["gt"][i], fmt="%.17g")


@pytest.fixture(scope="module")
def problem(tmp_path_factory):
    pb = synth.make_problem(5, 3000)
    d = tmp_path_factory.mktemp("voxel_data")
    write_dataset(str(d), pb)
    return pb, str(d)


def test_fused_model_is_voxel_grid_at_the_written_poses(problem, tmp_path):
    pb, d = problem
    o = tmp_path / "out"; o.mkdir()
    fused = str(tmp_path / "fused.xyz")
    subprocess.check_call([os.path.join(BIN, "multiview"), "--dir", d, "--out", str(o), "--rounds", "4", "--fused_out", fused, "--fused_voxel", "0.004"] + COMMON)
    rows = np.loadtxt(fused).reshape(-1, 6)
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(5)])
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        want = eng.voxel_grid(0.004, None, poses)
    finally:
        eng.close()
    assert len(rows) == len(want["cnt"]) > 1000
    assert np.ascontiguousarray(rows[:, :3]).tobytes() == want["xyz"].tobytes()
    assert np.ascontiguousarray(rows[:, 3:]).tobytes() == want["nrm"].tobytes()
    with open(fused) as f:
        assert sum(1 for _ in f) == len(rows)          # exactly m rows, no count line


def test_coarse_to_fine_matches_engine_sequence(problem, tmp_path):
    pb, d = problem
    o = tmp_path / "out"; o.mkdir()
    trace = str(tmp_path / "trace.txt")
    subprocess.check_call([os.path.join(BIN, "multiview"), "--dir", d, "--out", str(o), "--rounds", "4", "--coarse_voxel", "0.006", "--coarse_rounds", "2",
                           "--trace", trace] + COMMON)
    got = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(5)])
    # the same sequence through the binding: per-frame voxel_grid without poses -> a coarse engine for 2 rounds -> the full engine for 2
    # rounds from those poses, on the same graph (the driver's includes the fixed frame's own, inactive, edges)
    src, dst = synth.pose_graph_knn(pb["init"], 2, skip_fixed0=False)
    full, coarse = mvicp.Engine(0), mvicp.Engine(0)
    try:
        full.set_frames(pb["pts"], pb["nor"])
        levels = [full.voxel_grid(0.006, [i]) for i in range(5)]
        sizes = [len(lv["cnt"]) for lv in levels]
        assert all(0 < s < 3000 for s in sizes), sizes
        coarse.set_frames([lv["xyz"] for lv in levels], [lv["nrm"] for lv in levels]); coarse.set_graph(src, dst)
        full.set_graph(src, dst)
        poses = pb["init"].copy()
        for eng in (coarse, coarse, full, full):
            eng.correspond(poses, pb["fixed"], 0.05)
            poses, sm = eng.optimize(poses, pb["fixed"], L.PARAM_SOPHUS_SE3, 1, True, 50)
    finally:
        full.close(); coarse.close()
    assert np.allclose(got, poses, rtol=0, atol=1e-14), np.abs(got - poses).max()
    # the trace keeps its format; the per-edge counts of the coarse rounds cannot exceed the coarse clouds' sizes (and the fine rounds' do)
    C_lines = [ln.split() for ln in open(trace) if ln.startswith("C ")]
    P_lines = [ln.split() for ln in open(trace) if ln.startswith("P ")]
    assert len(C_lines) == 4 * len(src) and len(P_lines) == 4 * 5 and all(len(ln) == 7 for ln in C_lines) and all(len(ln) == 19 for ln in P_lines)
    fine_max = 0
    for _, r, i, j, dst_k, count, bits in C_lines:
        if int(r) < 2:
            assert int(count) <= sizes[int(i)], (r, i, j, count, sizes)
        else:
            fine_max = max(fine_max, int(count))
    assert fine_max > max(sizes)
    last = np.array([[float(v) for v in ln[3:]] for ln in P_lines[-5:]]).reshape(5, 4, 4)
    assert np.array_equal(last, got)
