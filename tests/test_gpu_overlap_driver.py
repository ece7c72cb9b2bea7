"""-m gpu: bin/multiview --graph overlap builds its pose graph from the overlap census (Session::computeOverlapNeighbours); without the
flag the driver prints and computes what it did before."""
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
K, N, ROUNDS = 6, 4000, 3


def write_dataset(d, pb):
    for i, (p, n) in enumerate(zip(pb["pts"], pb["nor"])):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([p, n]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), pb["init"][i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), pb["gt"][i], fmt="%.17g")


def run(d, o, extra):
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS),
           "--norecomputeNormals", "--drop_phantom_row"] + extra
    out = subprocess.check_output(cmd, timeout=300).decode().splitlines()
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    return out, poses


def matrix_lines(src, dst):
    A = np.zeros((K, K), dtype=int)
    A[src, dst] = 1
    return ["graph adjacency matrix == block structure"] + ["".join(f"{v} " for v in row) for row in A]


def stable(lines):
    """the driver's output without its wall-clock lines"""
    return [l for l in lines if not l.startswith("round: ") and not l.startswith("loop: ")]


def engine_loop(pb, src, dst, thresh=0.05):
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(src, dst)
        P = pb["init"].copy()
        for _ in range(ROUNDS):
            eng.correspond(P, pb["fixed"], thresh)
            P, _ = eng.optimize(P, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
    finally:
        eng.close()
    return P


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    pb = synth.make_problem(K, N, cone_deg=40)
    d = tmp_path_factory.mktemp("overlap_data")
    write_dataset(str(d), pb)
    return pb, d


@pytest.mark.parametrize("extra,cutoff,ms,minf", [([], 0.05, 4096, 0.0),
                                                  (["--overlap_cutoff", "0.01", "--overlap_samples", "1000", "--overlap_min", "0.2"], 0.01, 1000, 0.2),
                                                  (["--overlap_samples", "0", "--knn", "3"], 0.05, 0, 0.0)])
def test_overlap_graph_flag(dataset, tmp_path, extra, cutoff, ms, minf):
    pb, d = dataset
    knn = 3 if "--knn" in extra else 2
    out, poses = run(d, tmp_path, ["--graph", "overlap"] + extra)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        ov = eng.overlap(pb["init"], cutoff, ms)
    finally:
        eng.close()
    src, dst, nc = mvicp.graph_from_overlap(ov["samples"], ov["hits"], ov["sumq"], knn=knn, min_fraction=minf, skip_fixed0=False)
    assert len(src) > 0
    want = matrix_lines(src, dst) + [f"overlap graph: {nc} component(s)"]
    assert out[:len(want)] == want, "\n".join(out[:len(want) + 1])
    ref = engine_loop(pb, src, dst)
    assert np.allclose(poses, ref, rtol=0, atol=1e-14), np.abs(poses - ref).max()


def test_default_is_the_pose_graph(dataset, tmp_path):
    pb, d = dataset
    a = tmp_path / "a"; b = tmp_path / "b"
    a.mkdir(); b.mkdir()
    out_default, poses_default = run(d, a, [])
    out_pose, poses_pose = run(d, b, ["--graph", "pose"])
    assert stable(out_default) == stable(out_pose) and poses_default.tobytes() == poses_pose.tobytes()
    assert not any("overlap graph" in l for l in out_default)
    src, dst = synth.pose_graph_knn(pb["init"], 2, skip_fixed0=False)
    want = matrix_lines(src, dst)
    assert out_default[:len(want)] == want and out_default[len(want)].startswith("round: 0")
    ref = engine_loop(pb, src, dst)
    assert np.allclose(poses_default, ref, rtol=0, atol=1e-14), np.abs(poses_default - ref).max()
