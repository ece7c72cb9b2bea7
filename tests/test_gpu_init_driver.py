"""-m gpu: bin/multiview --init features starts a registration from the clouds alone (Session::initFromFeatures): its per-edge lines are
mvicp.init_from_clouds' counts, and after the rounds it stands where the run started AT the ground truth stands.  Without the flag the
driver prints and computes what it did before."""
import os
import re
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
K, ROUNDS, CUTOFF, SEED = 4, 20, 0.05, 12345
# the distance between the two runs' final poses measured on the MI355X, the largest over frames 1 - 3: 0.0019013 degrees and 0.0025348
# spacings (per frame 0.00159 / 0.00253, 0.00166 / 0.00062, 0.00190 / 0.00119; the run started at the truth itself ends within 0.036 deg and 0.09
# spacings of the truth).  The bound is three times the measured value, and below 1 degree / 1 spacing in any case.
MEASURED_DEG, MEASURED_SPACINGS = 0.0019013, 0.0025348


def write_dataset(d, cl, init):
    for i in range(K):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), init[i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")


def run(d, o, extra):
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS), "--cutoff", str(CUTOFF),
           "--knn", "3", "--norecomputeNormals", "--drop_phantom_row"] + extra
    out = subprocess.check_output(cmd, timeout=300).decode().splitlines()
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    return out, poses


def stable(lines):
    """the driver's output without its wall-clock lines"""
    return [l for l in lines if not l.startswith("round: ") and not l.startswith("loop: ")]


def matrix_lines(src, dst):
    A = np.zeros((K, K), dtype=int)
    A[src, dst] = 1
    return ["graph adjacency matrix == block structure"] + ["".join(f"{v} " for v in row) for row in A]


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """the fixture of tests/initref.py as two datasets with ground-truth files: pose files at the ground truth, and pose files that say
    nothing (the identity everywhere: frame 0's is its ground truth)"""
    cl = ir.fixture_clouds()
    at_truth, blank = tmp_path_factory.mktemp("init_truth"), tmp_path_factory.mktemp("init_blank")
    write_dataset(str(at_truth), cl, cl["gt"])
    write_dataset(str(blank), cl, np.tile(np.eye(4), (K, 1, 1)))
    return cl, at_truth, blank


def feature_flags(cl):
    return ["--init", "features", "--feat_min_count", str(ir.FIX_MIN_COUNT), "--feat_radius", repr(cl["radius"]), "--feat_tau", repr(cl["tau"]),
            "--feat_hyp", str(ir.FIX_H), "--feat_seed", str(SEED), "--feat_max_nn", str(ir.FIX_MAX_NN), "--feat_edge_sim", str(ir.FIX_EDGE_SIM)]


def test_feature_init_reaches_the_run_started_at_the_truth(datasets, tmp_path):
    """K = 4 with --knn 3 is the complete graph in both runs.  The run started at the ground truth is existing code and the yardstick; the
    initialisation itself is within 1.14 deg / 2.8 spacings of the truth (tests/test_init_cpu.py), so two runs that end within a fraction
    of a spacing of each other show that the refinement happened on top of it.  Measured on the MI355X: 0.0019 deg and 0.0025 spacings at
    the worst frame (MEASURED_* above); asserted: three times that."""
    cl, at_truth, blank = datasets
    a = tmp_path / "a"; b = tmp_path / "b"
    a.mkdir(); b.mkdir()
    out_f, poses_f = run(blank, a, ["--quiet"] + feature_flags(cl))
    out_t, poses_t = run(at_truth, b, ["--quiet"])
    # the per-edge lines are init_from_clouds' counts
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        want = mvicp.init_from_clouds(eng, list(range(K)), cl["xyz"], cl["radius"], cl["tau"], max_nn=ir.FIX_MAX_NN, hypotheses=ir.FIX_H, seed=SEED,
                                      edge_sim=ir.FIX_EDGE_SIM, min_count=ir.FIX_MIN_COUNT)
    finally:
        eng.close()
    lines = [f"feature init: edge {i} {j} pairs {r['pairs']} accepted {r['accepted']} inliers {r['inliers']}" for (i, j), r in zip(want["edges"].tolist(), want["records"])]
    lines.append(f"feature init: {want['components']} component(s)")
    assert [l for l in out_f if l.startswith("feature init")] == lines, "\n".join(out_f)
    assert want["components"] == 1 and sum(r["inliers"] >= ir.FIX_MIN_COUNT for r in want["records"]) >= K - 1
    assert not any(l.startswith("feature init") for l in out_t)
    worst_deg = worst_sp = 0.0
    for k in range(1, K):
        deg, dt = ir.pose_error(poses_f[k], poses_t[k])
        print("frame", k, "features vs truth start: deg", deg, "spacings", dt / cl["spacing"], "| truth start vs truth:", ir.pose_error(poses_t[k], cl["gt"][k]))
        worst_deg, worst_sp = max(worst_deg, deg), max(worst_sp, dt / cl["spacing"])
    print("worst", worst_deg, worst_sp)
    assert poses_f[0].tobytes() == poses_t[0].tobytes()
    bound_deg, bound_sp = min(3.0 * MEASURED_DEG, 1.0), min(3.0 * MEASURED_SPACINGS, 1.0)
    assert bound_deg < 1.0 + 1e-12 and bound_sp < 1.0 + 1e-12
    assert worst_deg <= bound_deg and worst_sp <= bound_sp, (worst_deg, worst_sp)


def test_feature_init_on_voxel_copies(datasets, tmp_path):
    """--feat_voxel H: Frame::voxelDownsample(H) copies carry the features; the per-edge lines are init_from_clouds' counts on the voxel
    grids of the frames, and the rounds then run on the full frames"""
    cl, _, blank = datasets
    H = 0.012
    out, poses = run(blank, tmp_path, ["--quiet", "--feat_voxel", str(H)] + feature_flags(cl))
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        levels = [eng.voxel_grid(H, [i]) for i in range(K)]
        assert all(100 < len(lv["cnt"]) < len(x) for lv, x in zip(levels, cl["xyz"])), [len(lv["cnt"]) for lv in levels]
        eng.set_frames([lv["xyz"] for lv in levels], [lv["nrm"] for lv in levels])
        want = mvicp.init_from_clouds(eng, list(range(K)), [lv["xyz"] for lv in levels], cl["radius"], cl["tau"], max_nn=ir.FIX_MAX_NN, hypotheses=ir.FIX_H,
                                      seed=SEED, edge_sim=ir.FIX_EDGE_SIM, min_count=ir.FIX_MIN_COUNT)
    finally:
        eng.close()
    lines = [f"feature init: edge {i} {j} pairs {r['pairs']} accepted {r['accepted']} inliers {r['inliers']}" for (i, j), r in zip(want["edges"].tolist(), want["records"])]
    lines.append(f"feature init: {want['components']} component(s)")
    assert [l for l in out if l.startswith("feature init")] == lines, "\n".join(out)
    assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()


def test_without_the_flag_nothing_changes(datasets, tmp_path):
    """the default run prints the adjacency matrix, the rounds, the loop line and one line per frame, no line of the initialisation, and
    ends where the same sequence of engine calls ends"""
    cl, at_truth, _ = datasets
    out, poses = run(at_truth, tmp_path, [])
    assert not any("feature init" in l for l in out)
    src, dst = synth.pose_graph_knn(cl["gt"], 3, skip_fixed0=False)
    want = matrix_lines(src, dst)
    assert out[:len(want)] == want and out[len(want)].startswith("round: 0")
    rest = stable(out)[len(want):]
    assert len(rest) >= K and all(re.match(r"frame %d\b" % i, l) for i, l in enumerate(l for l in rest if l.startswith("frame ")))
    assert sum(l.startswith("round: ") for l in out) == ROUNDS and sum(l.startswith("loop: ") for l in out) == 1
    fixed = np.array([1] + [0] * (K - 1), dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"]); eng.set_graph(src, dst)
        P = cl["gt"].copy()
        for _ in range(ROUNDS):
            eng.correspond(P, fixed, CUTOFF)
            P, _ = eng.optimize(P, fixed, L.PARAM_SOPHUS_SE3, True, True, 50)
    finally:
        eng.close()
    assert np.allclose(poses, P, rtol=0, atol=1e-14), np.abs(poses - P).max()
