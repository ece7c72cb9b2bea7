"""-m gpu: the plane flags of the headless driver (mv-lm-icp_amd/bin/multiview --plane_tau / --plane_hyp / --plane_seed / --plane_keep /
--plane_axis / --plane_cos), which is how Frame::removePlane is tested: the lines it prints are the reference's numbers, and the clouds it
registers are the reference's kept sets -- its final poses equal, byte for byte, those of a run without the flags on cloud files written
from those sets."""
import os
import re
import subprocess

import numpy as np
import pytest

import planeref as pr
from mvicp import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "mv-lm-icp_amd", "bin")
COMMON = ["--step", "1", "--limit", "40", "--quiet", "--norecomputeNormals", "--drop_phantom_row", "--rounds", "10"]
K_VIEWS, N_PTS, N_PATCH = 4, 3000, 1500
TAU, HYP, SEED = 0.004, 512, 3
NUM = r"(-?(?:\d+\.?\d*(?:e[-+]?\d+)?|inf|nan))"
LINE = r"^plane filter: frame (\d+) kept (\d+) of (\d+), (\d+) inliers, plane " + " ".join([NUM] * 4) + "$"


def _write(d, pb, pts, nor):
    for i in range(K_VIEWS):
        np.savetxt(os.path.join(d, f"cloud_{i}.xyz"), np.hstack([pts[i], nor[i]]), fmt="%.17g")
        np.savetxt(os.path.join(d, f"pose_{i}.txt"), pb["init"][i], fmt="%.17g")
        np.savetxt(os.path.join(d, f"groundtruth_{i}.txt"), pb["gt"][i], fmt="%.17g")


@pytest.fixture(scope="module")
def problem(tmp_path_factory):
    """4 views x 3000 points; into every view a planar patch of 1 500 points (0.3 x 0.3, sigma 1 mm) is planted at a random place of the
    index range: a support plane through a point 0.12 behind the view's centroid (5 cm under the surface at the nearest), tilted a little
    differently in every view."""
    pb = synth.make_problem(K_VIEWS, N_PTS)
    rng = np.random.Generator(np.random.PCG64(4343))
    pts, nor, planted = [], [], []
    for i, p in enumerate(pb["pts"]):
        at = int(rng.integers(1, len(p)))
        nv = np.array([0.0, 0.0, 1.0]) + rng.normal(0.0, 0.1, size=3)
        nv /= np.linalg.norm(nv)
        e1 = np.cross(nv, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
        e2 = np.cross(nv, e1)
        uv = rng.uniform(-0.15, 0.15, size=(N_PATCH, 2))
        patch = p.mean(0) - 0.12 * nv + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0.0, 0.001, size=(N_PATCH, 1)) * nv
        pts.append(np.vstack([p[:at], patch, p[at:]]))
        nor.append(np.vstack([pb["nor"][i][:at], np.tile(nv, (N_PATCH, 1)), pb["nor"][i][at:]]))
        planted.append(np.arange(at, at + N_PATCH))
    d = str(tmp_path_factory.mktemp("plane_data"))
    _write(d, pb, pts, nor)
    # the driver reads the files: the reference must see the bytes the files hold
    pts = [np.ascontiguousarray(np.loadtxt(os.path.join(d, f"cloud_{i}.xyz"))[:, :3]) for i in range(K_VIEWS)]
    nor = [np.ascontiguousarray(np.loadtxt(os.path.join(d, f"cloud_{i}.xyz"))[:, 3:]) for i in range(K_VIEWS)]
    return pb, pts, nor, planted, d


def _run(d, out, extra):
    os.makedirs(out)
    text = subprocess.check_output([os.path.join(BIN, "multiview"), "--dir", d, "--out", out] + COMMON + extra, universal_newlines=True)
    poses = np.array([np.loadtxt(os.path.join(out, f"pose_{i}.txt")) for i in range(K_VIEWS)])
    return text, poses


def _lines(text):
    return [(int(m[0]), int(m[1]), int(m[2]), int(m[3])) + tuple(np.float64(v).tobytes() for v in m[4:]) for m in re.findall(LINE, text, flags=re.M)]


def test_printed_lines_and_registration(problem, tmp_path):
    pb, pts, nor, planted, d = problem
    want, want_plane, rest, plane = [], [], [], []
    for p, nr, sel in zip(pts, nor, planted):   # on the reference alone: the planted patch goes, the surface stays
        r = pr.segment(p, nr, TAU, HYP, SEED)
        surface = np.setdiff1d(np.arange(len(p)), sel)
        assert r["refit"] == 1 and (r["flags"][sel] == 1).mean() >= 0.99 and (r["flags"][surface] == 1).mean() <= 0.01
        s, t = pr.select(p, nr, r, False), pr.select(p, nr, r, True)
        tail = (r["count_refined"],) + tuple(np.float64(v).tobytes() for v in (r["normal"][0], r["normal"][1], r["normal"][2], r["d"]))
        want.append((s["kept"], len(p)) + tail); want_plane.append((t["kept"], len(p)) + tail)
        rest.append(s); plane.append(t)
    plain_text, plain = _run(d, str(tmp_path / "plain"), [])
    assert "plane filter" not in plain_text                                           # default off
    flags = ["--plane_tau", str(TAU), "--plane_hyp", str(HYP), "--plane_seed", str(SEED)]
    text, clean = _run(d, str(tmp_path / "clean"), flags)
    assert _lines(text) == [(i,) + w for i, w in enumerate(want)], (text, want)
    # the same plane through --plane_keep plane; then with an axis, which rejects most hypotheses: the reference's numbers again
    text_p, _ = _run(d, str(tmp_path / "keep"), flags + ["--plane_keep", "plane"])
    assert _lines(text_p) == [(i,) + w for i, w in enumerate(want_plane)]
    axis_want = []
    for i, (p, nr) in enumerate(zip(pts, nor)):
        r = pr.segment(p, nr, TAU, HYP, SEED, axis=(0.0, 0.0, 1.0), cos_min=0.9)
        axis_want.append((i, pr.select(p, nr, r, False)["kept"], len(p), r["count_refined"]) + tuple(np.float64(v).tobytes() for v in (r["normal"][0], r["normal"][1], r["normal"][2], r["d"])))
        assert 0 < r["accepted"] < HYP
    text_a, _ = _run(d, str(tmp_path / "axis"), flags + ["--plane_axis=0,0,1", "--plane_cos", "0.9"])
    assert _lines(text_a) == axis_want
    # the clouds the driver registered are the reference's kept sets: a run without the flags on files written from them ends at the same poses
    d2 = str(tmp_path / "kept_data")
    os.makedirs(d2)
    _write(d2, pb, [s["xyz"] for s in rest], [s["nrm"] for s in rest])
    text_ref, ref = _run(d2, str(tmp_path / "ref"), [])
    assert "plane filter" not in text_ref
    assert clean.tobytes() == ref.tobytes()
    # distance to the ground truth with and without the filter: printed, not asserted (nobody has measured what the patch costs)
    err = lambda P: np.sum([synth.pose_diff(P[i], pb["gt"][i]) for i in range(K_VIEWS)], axis=0)
    print("pose_diff sums (dt, dr): without the flag", err(plain), "with", err(clean))
