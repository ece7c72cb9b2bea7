"""The 1-NN tie fix-up's walk (mv-lm-icp_amd/csrc/tie_walk.h — the function nn_tie.hip's kernels run), compiled for the host and held to the
REAL nanoflann's findNeighbors, index and squared distance, on: the Bunny golden pair (tests/golden/bunny_nn.npz), the lattice with
duplicates of tests/test_knn_tie_order.py, and DEEP clouds — coordinates in geometric progression plus duplicates, whose tree is as deep as
it has distinct points (200, 300 and 900 levels) and whose exact ties nanoflann decides by visit order.  nanoflann's answers on the deep
clouds are recorded in tests/golden/deep_tie_nn.npz (tests/golden/make_deep_tie_nn.py); where oracle/_ref is built, a live run must
reproduce the recording.  The GPU side of the same clouds is tests/test_gpu_deep_tie.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEEP_N = (200, 300, 900)
TRUNCATED = -2          # tie_walk.h TIE_WALK_TRUNCATED
OLD_STACK = 128         # nn_tie_kernel's per-lane stack (TIE_STACK)


def deep_cloud(n):
    """n points (x, 0, 0) with x = 2^-n/2 .. 2^(n/2 - 1), every third one twice, rows permuted: every middle split peels one point off."""
    x = 2.0 ** np.arange(-(n // 2), n - n // 2, dtype=np.float64)
    pts = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    pts = np.vstack([pts, pts[::3]])
    return np.ascontiguousarray(pts[np.random.default_rng(1).permutation(len(pts))])


def deep_queries(pts):
    """-> (self queries = the cloud, every d2 = 0; the same points moved aside along y by a quarter of their x: d2 = x^2 / 16, the nearest
    target still the point itself — and its duplicate, where it has one)."""
    aside = pts.copy()
    aside[:, 1] = 0.25 * pts[:, 0]
    return pts, aside


def lowest_index(pts, q):
    """The kernels' own rule (and the oracle's scan): the lowest index among the targets at the minimum distance, the metric's own sums."""
    e = q[:, None, :] - pts[None, :, :]
    d = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
    i = np.argmin(d, axis=1)          # (first occurrence of the minimum)
    return i.astype(np.int32), d[np.arange(len(q)), i]


def recording(refnn, n):
    """nanoflann's (idx, d2) for the self and the aside queries of deep_cloud(n), from the golden file; checked live where oracle/_ref is built."""
    G = np.load(os.path.join(GOLD, "deep_tie_nn.npz"))
    pts = deep_cloud(n)
    qs, qa = deep_queries(pts)
    out = {k: G[f"n{n}_{k}"] for k in ("self_idx", "self_d2", "aside_idx", "aside_d2")}
    if refnn is not None:
        for tag, q in (("self", qs), ("aside", qa)):
            i, d = refnn.query(pts, q)
            assert np.array_equal(i, out[tag + "_idx"]) and np.array_equal(d, out[tag + "_d2"]), (n, tag)
    return pts, qs, qa, out


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tiewalk") / "kdvisit_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mv-lm-icp_amd", "csrc"),
                           "-o", so, os.path.join(ROOT, "tests", "kdvisit_harness.cpp")])
    return C.CDLL(so)


def walk(lib, pts, q, cap=0):
    pts = np.ascontiguousarray(pts, dtype=np.float64); q = np.ascontiguousarray(q, dtype=np.float64)
    idx = np.zeros(len(q), dtype=np.int32); d2 = np.zeros(len(q), dtype=np.float64)
    levels = lib.tie_walk_emul(pts.ctypes.data_as(C.c_void_p), len(pts), q.ctypes.data_as(C.c_void_p), len(q), int(cap),
                               idx.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p))
    return idx, d2, levels


def test_walk_equals_nanoflann_on_the_bunny_golden_pair(harness):
    G = np.load(os.path.join(GOLD, "bunny_nn.npz"))
    for tag in ("gt", "noisy"):
        idx, d2, levels = walk(harness, G["dst"], G["q_" + tag])
        assert levels <= OLD_STACK                                      # an ordinary cloud: the per-lane stack holds its tree
        assert np.array_equal(idx, G["idx_" + tag]) and np.array_equal(d2, G["d2_" + tag]), tag


def test_walk_equals_nanoflann_on_the_lattice_with_duplicates(harness, refnn):
    import test_knn_tie_order as T
    pts = T.lattice_points()
    idx, d2, levels = walk(harness, pts, pts)
    want = np.load(os.path.join(GOLD, "deep_tie_nn.npz"))
    if refnn is not None:
        ri, rd = refnn.query(pts, pts)
        assert np.array_equal(ri, want["lattice_self_idx"]) and np.array_equal(rd, want["lattice_self_d2"])
    assert (want["lattice_self_idx"][:1000] != lowest_index(pts, pts[:1000])[0]).sum() > 50, "the lattice must make the two tie rules disagree"
    assert np.array_equal(idx, want["lattice_self_idx"]) and np.array_equal(d2, want["lattice_self_d2"])
    assert levels <= OLD_STACK


@pytest.mark.parametrize("n", DEEP_N)
def test_walk_equals_nanoflann_on_deep_trees(harness, refnn, n):
    pts, qs, qa, want = recording(refnn, n)
    for tag, q in (("self", qs), ("aside", qa)):
        idx, d2, levels = walk(harness, pts, q)                          # a stack of the levels the builder reports: what the product allocates
        assert levels == n                                              # one level per distinct coordinate
        assert np.array_equal(idx, want[tag + "_idx"]) and np.array_equal(d2, want[tag + "_d2"]), (n, tag, int((idx != want[tag + "_idx"]).sum()))
        short, _, _ = walk(harness, pts, q, cap=levels - 1)             # the bound is tight: one entry fewer truncates some walk — and says so
        assert (short == TRUNCATED).any()
        ok = short != TRUNCATED
        assert np.array_equal(short[ok], want[tag + "_idx"][ok])


@pytest.mark.parametrize("n", [300, 900])
def test_deep_clouds_defeat_a_128_entry_stack(harness, n):
    """Input condition, from the recording and the committed walk alone: nanoflann's answer differs from the lowest index on at least 30 self
    queries whose walk needs more than 127 pending entries — the queries a 128-entry stack that gives up silently leaves wrong."""
    pts = deep_cloud(n)
    qs, qa = deep_queries(pts)
    G = np.load(os.path.join(GOLD, "deep_tie_nn.npz"))
    for tag, q, least in (("self", qs, 30), ("aside", qa, 30)):
        want = G[f"n{n}_{tag}_idx"]
        low, d = lowest_index(pts, q)
        assert np.array_equal(d, G[f"n{n}_{tag}_d2"])
        short, _, _ = walk(harness, pts, q, cap=OLD_STACK)
        differ = want != low
        hit = differ & (short == TRUNCATED)
        print(f"deep n={n} {tag}: {len(q)} queries, nanoflann != lowest index on {int(differ.sum())}, of those {int(hit.sum())} need more than {OLD_STACK - 1} pending entries; "
              f"{int((short == TRUNCATED).sum())} walks truncated in all")
        assert hit.sum() >= least, (n, tag, int(differ.sum()), int(hit.sum()))
