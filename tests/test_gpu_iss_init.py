"""-m gpu: the clouds-alone initialisation on ISS keypoints.  mvicp.init_from_clouds(keypoints=...) equals the CPU chain issref ->
fpfhref -> initref.coarse_edge -> poses_from_pairs in every record, pair, flag and pose, in both modes; keypoints=None is the path it was;
bin/multiview --init features --feat_keypoints iss|iss_src prints the counts of the Python chain and runs its rounds from there."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fpfhref
import initref as ir
import issref
import mvicp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
K, SEED, MIN_COUNT, TAU_SPACINGS = 4, 12345, 3, 3.0
# chosen on the CPU (tests/issref.py chain on fixture_clouds(1500)): one component and at least 18 pairs on every edge in both modes --
# "both": 90 / 77 / 89 / 82 keypoints, pairs 35, 34, 25, 36, 24, 33, inliers 4, 4, 3, 4, 4, 7; "src": pairs 68, 65, 52, 63, 59, 70, inliers
# 12, 8, 4, 13, 6, 27
KP = (0.6, 0.25, 0.975, 0.975, 5)


def kp_params(cl):
    return (KP[0] * cl["radius"], KP[1] * cl["radius"]) + KP[2:]


def kp_dict(cl, mode):
    rs, rn, g21, g32, mn = kp_params(cl)
    return {"salient_radius": rs, "non_max_radius": rn, "gamma21": g21, "gamma32": g32, "min_neighbors": mn, "mode": mode}


@functools.lru_cache(maxsize=None)
def descriptors():
    cl = ir.fixture_clouds()
    return [fpfhref.fpfh(cl["xyz"][k], cl["nrm"][k], cl["radius"], ir.FIX_MAX_NN)["desc"] for k in range(K)]


@functools.lru_cache(maxsize=None)
def reference(mode):
    cl = ir.fixture_clouds()
    return issref.chain(cl["xyz"], descriptors(), ir.FIX_EDGES, kp_params(cl), mode, TAU_SPACINGS * cl["spacing"], ir.FIX_H,
                        [SEED + e for e in range(len(ir.FIX_EDGES))], ir.FIX_EDGE_SIM, MIN_COUNT)


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def init(eng, cl, mode, refine):
    return mvicp.init_from_clouds(eng, list(range(K)), cl["xyz"], cl["radius"], TAU_SPACINGS * cl["spacing"], max_nn=ir.FIX_MAX_NN, hypotheses=ir.FIX_H, seed=SEED,
                                  edge_sim=ir.FIX_EDGE_SIM, min_count=MIN_COUNT, refine=refine, keypoints=None if mode is None else kp_dict(cl, mode))


@pytest.mark.parametrize("mode", ["both", "src"])
def test_init_on_keypoints_equals_the_cpu_chain(eng, mode):
    cl, ref = ir.fixture_clouds(), reference(mode)
    assert ref["tree"]["components"] == 1 and min(e["pairs_n"] for e in ref["edges"]) >= 3 and min(len(k) for k in ref["keypoints"]) > 20
    assert sum(e["count"] >= MIN_COUNT for e in ref["edges"]) >= K - 1
    eng.set_frames(cl["xyz"], cl["nrm"])
    out = init(eng, cl, mode, False)
    assert [k.tobytes() for k in out["keypoints"]] == [k.tobytes() for k in ref["keypoints"]]
    assert [tuple(e) for e in out["edges"].tolist()] == list(ir.FIX_EDGES)
    for e, (rec, want) in enumerate(zip(out["records"], ref["edges"])):
        assert (rec["pairs"], rec["accepted"], rec["inliers"], rec["best"]) == (want["pairs_n"], want["accepted"], want["count"], want["best"]), e
        assert rec["pose"].tobytes() == want["pose"].tobytes(), e
        pairs, flags = eng.coarse_pairs_fetch(e)
        assert pairs.tobytes() == want["pairs"].tobytes() and flags.tobytes() == want["flags"].tobytes(), e
    for key in ("poses", "parent", "parent_edge", "component"):
        assert out[key].tobytes() == ref["tree"][key].tobytes(), key
    assert out["components"] == 1
    # with the refinement the counts, and so the tree, are the same, and each refined tree edge is the closed form over the matched rows
    fine = init(eng, cl, mode, True)
    for key in ("parent", "parent_edge", "component"):
        assert fine[key].tobytes() == ref["tree"][key].tobytes(), key
    for e, ((i, j), rec, want) in enumerate(zip(ir.FIX_EDGES, fine["records"], ref["edges"])):
        if want["count"] >= 3:
            keep = want["flags"] != 0
            rows_i = cl["xyz"][i][ref["keypoints"][i]]
            rows_j = cl["xyz"][j][ref["keypoints"][j]] if mode == "both" else cl["xyz"][j]
            closed = mvicp.lib.closedform_point_to_point(rows_i[want["pairs"][keep, 0]], rows_j[want["pairs"][keep, 1]])
            assert rec["refined"].tobytes() == closed.tobytes(), e
        else:
            assert rec["refined"].tobytes() == want["pose"].tobytes(), e


def test_without_keypoints_the_path_is_unchanged(eng):
    """the call of tests/test_gpu_coarse.py test_init_from_clouds_in_one_call with keypoints=None spelled out"""
    cl, ref = ir.fixture_clouds(300), ir.fixture_reference(300)
    eng.set_frames(cl["xyz"], cl["nrm"])
    out = mvicp.init_from_clouds(eng, [0, 1, 2, 3], cl["xyz"], cl["radius"], cl["tau"], hypotheses=500, seed=77, min_count=3, refine=False, keypoints=None)
    assert "keypoints" not in out
    want = [ir.coarse_edge(ref["desc"][i], cl["xyz"][i], ref["desc"][j], cl["xyz"][j], True, 1.0, 500, 77 + e, cl["tau"], 0.9) for e, (i, j) in enumerate(ir.FIX_EDGES)]
    for rec, w in zip(out["records"], want):
        assert (rec["pairs"], rec["accepted"], rec["inliers"], rec["best"]) == (w["pairs_n"], w["accepted"], w["count"], w["best"])
        assert rec["pose"].tobytes() == w["pose"].tobytes()
    tree = ir.poses_from_pairs(4, [e[0] for e in ir.FIX_EDGES], [e[1] for e in ir.FIX_EDGES], [w["count"] for w in want], np.array([w["pose"] for w in want]), 3, 0)
    for key in ("poses", "parent", "parent_edge", "component"):
        assert out[key].tobytes() == tree[key].tobytes(), key


# ---- the driver
ROUNDS, CUTOFF = 20, 0.05


def write_dataset(d, cl, init_poses):
    for i in range(K):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([cl["xyz"][i], cl["nrm"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), init_poses[i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), cl["gt"][i], fmt="%.17g")


def run(d, o, extra):
    cmd = [os.path.join(BIN, "multiview"), "--dir", str(d), "--out", str(o), "--step", "1", "--limit", "40", "--rounds", str(ROUNDS), "--cutoff", str(CUTOFF),
           "--knn", "3", "--norecomputeNormals", "--drop_phantom_row", "--quiet"] + extra
    out = subprocess.check_output(cmd, timeout=300).decode().splitlines()
    poses = np.array([np.loadtxt(os.path.join(str(o), f"pose_{i}.txt")) for i in range(K)])
    return out, poses


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    cl = ir.fixture_clouds()
    at_truth, blank = tmp_path_factory.mktemp("iss_truth"), tmp_path_factory.mktemp("iss_blank")
    write_dataset(str(at_truth), cl, cl["gt"])
    write_dataset(str(blank), cl, np.tile(np.eye(4), (K, 1, 1)))
    return cl, at_truth, blank


def feature_flags(cl):
    return ["--init", "features", "--feat_min_count", str(MIN_COUNT), "--feat_radius", repr(cl["radius"]), "--feat_tau", repr(TAU_SPACINGS * cl["spacing"]),
            "--feat_hyp", str(ir.FIX_H), "--feat_seed", str(SEED), "--feat_max_nn", str(ir.FIX_MAX_NN), "--feat_edge_sim", str(ir.FIX_EDGE_SIM)]


def keypoint_flags(cl, which):
    rs, rn, g21, g32, mn = kp_params(cl)
    return ["--feat_keypoints", which, "--feat_salient_radius", repr(rs), "--feat_nms_radius", repr(rn), "--feat_gamma21", repr(g21), "--feat_gamma32", repr(g32),
            "--feat_min_neighbors", str(mn)]


@pytest.fixture(scope="module")
def truth_run(datasets, tmp_path_factory):
    cl, at_truth, _ = datasets
    return run(at_truth, tmp_path_factory.mktemp("iss_truth_out"), [])[1]


@pytest.mark.parametrize("which", ["iss", "iss_src"])
def test_driver_on_keypoints(eng, datasets, truth_run, tmp_path, which):
    cl, _, blank = datasets
    out, poses = run(blank, tmp_path, feature_flags(cl) + keypoint_flags(cl, which))
    eng.set_frames(cl["xyz"], cl["nrm"])
    want = init(eng, cl, "both" if which == "iss" else "src", True)
    lines = [f"feature init: frame {i} keypoints {len(k)} of {len(x)}" for i, (k, x) in enumerate(zip(want["keypoints"], cl["xyz"]))]
    lines += [f"feature init: edge {i} {j} pairs {r['pairs']} accepted {r['accepted']} inliers {r['inliers']}" for (i, j), r in zip(want["edges"].tolist(), want["records"])]
    lines.append(f"feature init: {want['components']} component(s)")
    assert [l for l in out if l.startswith("feature init")] == lines, "\n".join(out)
    assert np.isfinite(poses).all() and poses[0].tobytes() == cl["gt"][0].tobytes()
    for k in range(1, K):   # printed, not asserted: how far the rounds end from the run started at the truth
        deg, dt = ir.pose_error(poses[k], truth_run[k])
        print(which, "frame", k, "vs the run started at the truth: deg", deg, "spacings", dt / cl["spacing"])


def test_driver_without_the_flag(datasets, tmp_path):
    """--feat_keypoints none is the default, and the default prints no keypoint line and ends at the same poses"""
    cl, _, blank = datasets
    a = tmp_path / "a"; b = tmp_path / "b"
    a.mkdir(); b.mkdir()
    out_a, poses_a = run(blank, a, feature_flags(cl))
    out_b, poses_b = run(blank, b, feature_flags(cl) + ["--feat_keypoints", "none"])
    feat = [l for l in out_a if l.startswith("feature init")]
    assert feat == [l for l in out_b if l.startswith("feature init")] and len(feat) == len(ir.FIX_EDGES) + 1
    assert not any("keypoints" in l for l in out_a) and poses_a.tobytes() == poses_b.tobytes()
    bad = subprocess.run([os.path.join(BIN, "multiview"), "--dir", str(blank), "--quiet", "--step", "1", "--init", "features", "--feat_keypoints", "harris"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert bad.returncode == 1 and b"feat_keypoints" in bad.stderr
