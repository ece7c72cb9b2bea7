"""-m gpu: bin/multiview --gicp [--gicp_epsilon E] runs the solves on the plane-to-plane objective (mvicp_optimize_gicp) in the parameterisation
the other flags select.  On the four-view fixture of tests/test_gpu_init_driver.py, started at the ground truth, with the fixture's own
normals: the run's final poses equal, byte for byte, those of the same loop driven through Engine, and the last of the 20 rounds moves less
than the first.  --gicp together with --symmetric is refused.  Distances from the truth are printed, not asserted: with the fixture's own
normals and with --normals_nn 16 --normals_fit 3 --normals_orient mst, next to the symmetric run's on the same normals."""
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
K, ROUNDS, CUTOFF, EPS = 4, 20, 0.05, 1e-3
FITTED = ["--normals_nn", "16", "--normals_fit", "3", "--normals_orient", "mst"]


def run(d, o, extra):
    trace = os.path.join(str(o), "trace.txt")
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS), "--cutoff", str(CUTOFF),
           "--knn", "3", "--drop_phantom_row", "--quiet", "--trace", trace] + extra
    subprocess.check_output(cmd, timeout=300)
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    per_round = {}
    for line in open(trace):
        w = line.split()
        if w[0] == "P":
            per_round[(int(w[1]), int(w[2]))] = np.array(w[3:], dtype=np.float64).reshape(4, 4)
    return poses, per_round


def engine_loop(cl):
    """the fixture's own normals, the driver's graph, 20 rounds of correspond + optimize_gicp -> poses"""
    src, dst = synth.pose_graph_knn(cl["gt"], 3, skip_fixed0=False)
    fixed = np.array([1] + [0] * (K - 1), dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(cl["xyz"], cl["nrm"])
        eng.set_graph(src, dst)
        P = cl["gt"].copy()
        for _ in range(ROUNDS):
            eng.correspond(P, fixed, CUTOFF)
            P, _ = eng.optimize_gicp(P, fixed, L.PARAM_SOPHUS_SE3, EPS, True, 50)
        return np.ascontiguousarray(P)
    finally:
        eng.close()


def _moved(a, b, cl):
    """largest (degrees, spacings) between two sets of poses over frames 1..K-1"""
    deg = sp = 0.0
    for k in range(1, K):
        e = ir.pose_error(a[k], b[k])
        deg, sp = max(deg, e[0]), max(sp, e[1] / cl["spacing"])
    return deg, sp


def test_gicp_driver_run_equals_the_engine_loop_and_settles(tmp_path):
    cl = ir.fixture_clouds()
    d = tmp_path / "data"
    d.mkdir()
    for i in range(K):
        np.savetxt(os.path.join(str(d), f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"pose_{i}.txt"), cl["gt"][i], fmt="%.17g")
        np.savetxt(os.path.join(str(d), f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")
    runs = {}
    for name, extra in (("gicp, own normals", ["--norecomputeNormals", "--gicp"]),
                        ("symmetric, own normals", ["--norecomputeNormals", "--symmetric"]),
                        ("gicp, fitted normals", FITTED + ["--gicp", "--gicp_epsilon", str(EPS)]),
                        ("symmetric, fitted normals", FITTED + ["--symmetric"])):
        o = tmp_path / name.replace(", ", "_").replace(" ", "_")
        o.mkdir()
        runs[name] = run(d, o, extra)
        poses, tr = runs[name]
        assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
        deg, sp = _moved(poses, cl["gt"], cl)
        last = _moved([tr[(ROUNDS - 1, k)] for k in range(K)], [tr[(ROUNDS - 2, k)] for k in range(K)], cl)
        print("driver %-26s ends %.5f deg, %.5f spacings from the truth; the last round moved %.2e deg, %.2e spacings" % (name, deg, sp, last[0], last[1]))
    poses, tr = runs["gicp, own normals"]
    P = engine_loop(cl)
    print("driver against the engine loop: largest difference of a pose entry %.3e" % np.abs(poses - P).max())
    assert poses.tobytes() == P.tobytes()
    first = _moved([tr[(0, k)] for k in range(K)], cl["gt"], cl)
    last = _moved([tr[(ROUNDS - 1, k)] for k in range(K)], [tr[(ROUNDS - 2, k)] for k in range(K)], cl)
    print("the first round moved %.2e deg, %.2e spacings; the last %.2e deg, %.2e spacings" % (first + last))
    assert last[0] < first[0] and last[1] < first[1], (first, last)
    assert poses.tobytes() != runs["symmetric, own normals"][0].tobytes()      # the flag selects another objective


def test_gicp_together_with_symmetric_is_refused(tmp_path):
    r = subprocess.run([os.path.join(BIN, "multiview"), "--dir", str(tmp_path), "--quiet", "--gicp", "--symmetric"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0 and b"--gicp" in r.stderr and b"--symmetric" in r.stderr
