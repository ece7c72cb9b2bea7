"""Row f1 (Frame::recomputeNormals -> getNeighbours -> nanoflann knnSearch, frame.cpp:208-255) on the reference's own lattice data, CPU
side: the product's tie rule (mv-lm-icp_amd/csrc/kdvisit.h — nanoflann's split structure restated + "the child on the query's side is
visited first") must reproduce the REAL nanoflann's 10-NN lists element for element, order included, on every row of
samples/Bunny_RealData/cloudXYZ_0.xyz (golden: tests/golden/bunny_knn_full.npz, 1185 of 16 264 points have a tie at the 10th place),
and on a synthetic lattice with duplicate points (golden: tests/golden/nanoflann_synthetic.npz, checked live where oracle/_ref is built).  The device kernel uses the same header
(tests/test_gpu_parity.py::test_recompute_normals_full_cloud_matches_nanoflann_lists)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kdv") / "kdvisit_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mv-lm-icp_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "kdvisit_harness.cpp")])
    return C.CDLL(so)


def knn(lib, pts, k):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.zeros((len(pts), k), dtype=np.int32)
    nodes = lib.knn_emul(pts.ctypes.data_as(C.c_void_p), len(pts), k, out.ctypes.data_as(C.c_void_p))
    return out, nodes


def test_tie_order_reproduces_nanoflann_lists_on_the_bunny_lattice(harness):
    pts = np.load(os.path.join(GOLD, "pairwise_kat.npz"))["pts"]          # every row of cloudXYZ_0.xyz
    G = np.load(os.path.join(GOLD, "bunny_knn_full.npz"))
    got, nodes = knn(harness, pts, 10)
    assert nodes == 2 * len(pts) - 1                                       # leaf size 1: a full binary tree
    assert G["tie_at_k"].sum() > 1000                                      # the data really is tie-ridden
    assert np.array_equal(got, G["knn_idx"])                               # same neighbours in the same order, all 16 264 points
    # what a lowest-index rule would have done instead (recorded for INTEGRATION.md): 3.6 % of the points get another neighbour set
    e = pts[:2000, None, :] - pts[None, :, :]
    d = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
    low = np.argsort(d, axis=1, kind="stable")[:, :10]
    differ = 1.0 - np.all(np.sort(low, axis=1) == np.sort(G["knn_idx"][:2000], axis=1), axis=1).mean()
    assert 0.005 < differ < 0.1, differ


def lattice_points():
    rng = np.random.default_rng(1)
    return np.round(rng.uniform(0, 1, (4000, 3)) * 20) / 20.0              # 21^3 lattice sites for 4000 points: duplicates and ties everywhere


def degenerate_points():
    x = 2.0 ** np.arange(-450, 450, dtype=np.float64)                     # (squared distances stay finite)
    pts = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    return np.vstack([pts, pts[::7]])                                   # + duplicates


def nanoflann_lists(refnn, name, pts):
    """The real nanoflann's 10-NN lists of `pts`: recorded in tests/golden/nanoflann_synthetic.npz (tests/golden/make_synthetic_nn.py);
    where oracle/_ref is built, a live run must reproduce the recording."""
    want = np.load(os.path.join(GOLD, "nanoflann_synthetic.npz"))[name]
    if refnn is not None:
        gi, _ = refnn.knn_self(pts, 10)
        assert np.array_equal(gi, want)
    return want


def test_tie_order_on_a_lattice_with_duplicate_points(harness, refnn):
    pts = lattice_points()
    gi = nanoflann_lists(refnn, "lattice_knn_idx", pts)
    got, _ = knn(harness, pts, 10)
    assert np.array_equal(got, gi)


def test_degenerate_depth_is_not_a_recursion_depth(harness, refnn):
    """A cloud whose coordinates form a geometric progression: every middle split (nanoflann.hpp:1034-1078) peels ONE point off, so the
    tree is as deep as it has points (900 levels here; the exponent range of a double allows ~2000).  The product's builder walks it with an explicit
    stack (kdvisit.h divide) and must still agree with the real nanoflann (which recurses that deep), ties and all."""
    pts = degenerate_points()
    gi = nanoflann_lists(refnn, "degenerate_knn_idx", pts)
    got, nodes = knn(harness, pts, 10)
    assert nodes == 2 * len(pts) - 1
    assert np.array_equal(got, gi)
