"""-m gpu: exact distance ties on DEEP trees through the 1-NN tie fix-up (mv-lm-icp_amd/csrc/nn_tie.hip).

The clouds of tests/test_tie_walk_cpu.py — coordinates in geometric progression plus duplicates — have a nanoflann tree of 200, 300 and
900 levels, and nanoflann decides their exact ties by visit order.  The fix-up's walk holds one pending subtree per level: a per-lane stack
of 128 entries that gave up silently left 44 of the 400 self queries at n = 300, and 202 of 1200 at n = 900, with the kernels' lowest-index
pick (tests/test_tie_walk_cpu.py::test_deep_clouds_defeat_a_128_entry_stack asserts the input condition).  Brute-force search plus the
fix-up isolates nn_tie_kernel / nn_tie_deep_kernel: index and squared distance must equal the REAL nanoflann's, recorded in
tests/golden/deep_tie_nn.npz (a live run must reproduce the recording where oracle/_ref is built).

The coordinates of these clouds span 2^-450 .. 2^449, outside float.  Besides NN_BRUTE only the raw-query grid search (nn_grid_kernel's
hash block + nn_far_kernel's box-tree descent, what mvicp_nn_query runs for NN_GRID / NN_TILE / NN_AUTO) goes on the GPU with them: its
loops are bounded on any finite input.  The edge path of the grid and tile kernels (cell staging, matrix-pipe
operands in f16) is not run on these clouds: their termination on such input has not been established by reading."""
import numpy as np
import pytest

import mvicp
from mvicp import lib as L
import test_tie_walk_cpu as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n", W.DEEP_N)
def test_nn_query_on_deep_trees_equals_nanoflann(eng, orc, refnn, n):
    pts, qs, qa, want = W.recording(refnn, n)
    eng.set_frames([pts], None)
    try:
        for tag, q in (("self", qs), ("aside", qa)):
            idx, d2 = eng.nn_query(0, q, L.NN_BRUTE)
            bad = int((idx != want[tag + "_idx"]).sum())
            print(f"deep n={n} {tag}: {bad} of {len(q)} indices differ from nanoflann")
            assert np.array_equal(d2, want[tag + "_d2"]), (n, tag)
            assert bad == 0, (n, tag, bad)
        # the rule switched off: the kernels' own pick, the oracle's lowest index
        eng.set_option("tie_rule", 0)
        for q in (qs, qa):
            idx, d2 = eng.nn_query(0, q, L.NN_BRUTE)
            oi, od = orc.nn_brute(pts, q)
            assert np.array_equal(idx, oi) and np.array_equal(d2, od), n
            assert np.array_equal(oi, W.lowest_index(pts, q)[0])
    finally:
        eng.set_option("tie_rule", 1)


@pytest.mark.parametrize("n", W.DEEP_N)
def test_grid_query_on_deep_trees_equals_nanoflann_or_refuses(eng, refnn, n):
    """The raw-query grid search on the same clouds: the recording, or an error status that leaves the context usable — never another answer."""
    pts, qs, qa, want = W.recording(refnn, n)
    eng.set_frames([pts], None)
    for tag, q in (("self", qs), ("aside", qa)):
        try:
            idx, d2 = eng.nn_query(0, q, L.NN_GRID)
        except mvicp.MvicpError as ex:
            print(f"deep n={n} {tag}: NN_GRID refused: {ex}")
            idx, d2 = eng.nn_query(0, q, L.NN_BRUTE)       # the context is still usable
        bad = int((idx != want[tag + "_idx"]).sum())
        print(f"deep n={n} {tag} (grid): {bad} of {len(q)} indices differ from nanoflann")
        assert np.array_equal(d2, want[tag + "_d2"]), (n, tag)
        assert bad == 0, (n, tag, bad)


@pytest.mark.parametrize("n", W.DEEP_N)
@pytest.mark.parametrize("lazy", [1, 0])
def test_correspond_on_deep_trees_equals_nanoflann(orc, refnn, n, lazy):
    """One edge, source = destination = the cloud, identity poses: every query is a point of the target (d2 = 0, every row accepted), and
    `second` is nanoflann's pick on every row — through the lazy tree build (the search repeated once) and the eager one."""
    pts, qs, qa, want = W.recording(refnn, n)
    e = mvicp.Engine(0)
    try:
        e.set_option("tie_lazy", lazy)
        e.set_frames([pts, pts], None); e.set_graph([1], [0])
        P = np.array([np.eye(4), np.eye(4)]); fixed = np.array([1, 0], dtype=np.uint8)
        for rep in range(2):                                   # (the second search meets the history of the first)
            c, w = e.correspond(P, fixed, 0.05, L.NN_BRUTE)
            f, s, d = e.get_correspondences(0)
            assert c[0] == len(pts) and np.array_equal(f, np.arange(len(pts))) and np.all(d == 0.0), (n, rep)
            bad = int((s != want["self_idx"]).sum())
            print(f"deep n={n} lazy={lazy} search {rep}: {bad} of {len(s)} `second` differ from nanoflann")
            assert bad == 0, (n, rep, bad)
        e.set_option("tie_rule", 0)
        c, w = e.correspond(P, fixed, 0.05, L.NN_BRUTE)
        f, s, d = e.get_correspondences(0)
        lo = orc.correspond_edge(pts, P[1], pts, P[0], 0.05)[1]
        assert np.array_equal(s, lo) and np.array_equal(lo, W.lowest_index(pts, pts)[0]), n
        assert not np.array_equal(lo, want["self_idx"])
    finally:
        e.close()
