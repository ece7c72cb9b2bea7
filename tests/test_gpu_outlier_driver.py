"""-m gpu: the outlier flags of the headless driver (mv-lm-icp_amd/bin/multiview --sor_k / --sor_ratio / --ror_radius): the clouds it
registers are the reference's kept sets, and cleaning clouds with planted off-surface points does not make the registration worse."""
import os
import re
import subprocess

import numpy as np
import pytest

import outlierref
from mvicp import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
COMMON = ["--step", "1", "--limit", "40", "--quiet", "--norecomputeNormals", "--drop_phantom_row", "--rounds", "10"]
K_VIEWS, N_PTS, SOR_K = 4, 3000, 8


@pytest.fixture(scope="module")
def problem(tmp_path_factory):
    """4 views x 3000 points; in every view 5 % of the points are lifted 1.5 - 3.5 cm off the surface along their normal: inside the
    search cutoff of 5 cm, so that they do find correspondences."""
    pb = synth.make_problem(K_VIEWS, N_PTS)
    rng = np.random.Generator(np.random.PCG64(4242))
    d = str(tmp_path_factory.mktemp("outlier_data"))
    pts, planted = [], []
    for i, p in enumerate(pb["pts"]):
        p = p.copy()
        sel = np.sort(rng.choice(len(p), size=len(p) // 20, replace=False))
        p[sel] += pb["nor"][i][sel] * rng.uniform(0.015, 0.035, size=(len(sel), 1))
        pts.append(p); planted.append(sel)
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([p, pb["nor"][i]]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), pb["init"][i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), pb["gt"][i], fmt="%.17g")
    return pb, pts, planted, d


def _run(d, out, extra):
    os.makedirs(out)
    text = subprocess.check_output([os.path.join(BIN, "multiview"), "--dir", d, "--out", out] + COMMON + extra, universal_newlines=True)
    poses = np.array([np.loadtxt(os.path.join(out, f"pose_{i}.txt")) for i in range(K_VIEWS)])
    return text, poses


def test_kept_counts_and_registration(problem, tmp_path):
    pb, pts, planted, d = problem
    want = [outlierref.outlier_filter(p, None, SOR_K, 2.0, 0.0) for p in pts]
    for w, sel in zip(want, planted):   # on the reference alone: the rule removes the planted points and little else
        removed = set(range(N_PTS)) - set(w["idx"].tolist())
        assert len(removed & set(sel.tolist())) >= 0.85 * len(sel) and len(removed) <= 2 * len(sel), (len(removed), len(sel))
    plain_text, plain = _run(d, str(tmp_path / "plain"), [])
    assert "outlier filter" not in plain_text                                         # default off
    text, clean = _run(d, str(tmp_path / "clean"), ["--sor_k", str(SOR_K), "--sor_ratio", "2"])
    lines = re.findall(r"^outlier filter: frame (\d+) kept (\d+) of (\d+)$", text, flags=re.M)
    assert [tuple(int(v) for v in ln) for ln in lines] == [(i, w["stats"]["kept"], N_PTS) for i, w in enumerate(want)]
    # the radius rule through the driver: the statistical rule is off when only a radius is given
    text_r, _ = _run(d, str(tmp_path / "radius"), ["--sor_k", str(SOR_K), "--ror_radius", "0.012"])
    want_r = [outlierref.outlier_filter(p, None, SOR_K, -1.0, 0.012)["stats"]["kept"] for p in pts]
    lines = re.findall(r"^outlier filter: frame (\d+) kept (\d+) of (\d+)$", text_r, flags=re.M)
    assert [int(ln[1]) for ln in lines] == want_r and all(0 < k < N_PTS for k in want_r)
    # pose_diff to ground truth (translation, rotation), summed over the views: no larger with the flags than without
    err = lambda P: np.sum([synth.pose_diff(P[i], pb["gt"][i]) for i in range(K_VIEWS)], axis=0)
    e_plain, e_clean = err(plain), err(clean)
    print("pose_diff sums (dt, dr): without the flags", e_plain, "with", e_clean)
    assert e_clean[0] <= e_plain[0] and e_clean[1] <= e_plain[1], (e_plain, e_clean)
