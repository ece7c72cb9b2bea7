"""Host side of the overlap census: the graph rule (mvicp_graph_from_overlap), the sample rule, and the argument check of mvicp_overlap
that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import mvicp
from mvicp import lib as L


def graph(samples, hits, sumq=None, **kw):
    src, dst, nc = mvicp.graph_from_overlap(samples, hits, sumq, **kw)
    return list(zip(src.tolist(), dst.tolist())), nc


def chain_table(K, strong=900, weak=300):
    h = np.zeros((K, K), dtype=np.int32)
    for i in range(K):
        h[i, i] = 1000
        for j in range(K):
            if abs(i - j) == 1:
                h[i, j] = strong
            elif abs(i - j) == 2:
                h[i, j] = weak
    return np.full(K, 1000, dtype=np.int32), h


def test_ranking_by_hits_and_edge_order():
    s, h = chain_table(5)
    h[2, 3] = 950   # frame 2: 3 before 1
    edges, nc = graph(s, h, knn=2, skip_fixed0=False)
    assert edges == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 3), (2, 1), (3, 2), (3, 4), (4, 3), (4, 2)]
    assert nc == 1
    edges0, nc0 = graph(s, h, knn=2, skip_fixed0=True)
    assert edges0 == edges[2:] and nc0 == 1
    assert graph(s, h, knn=1, skip_fixed0=True)[0] == [(1, 0), (2, 3), (3, 2), (4, 3)]


def test_sumq_breaks_ties_exactly_near_2_62():
    s = np.full(4, 100, dtype=np.int32)
    h = np.zeros((4, 4), dtype=np.int32)
    h[1, 0] = h[1, 2] = h[1, 3] = 50
    big = 1 << 62
    sq = np.zeros((4, 4), dtype=np.int64)
    sq[1, 0] = big + 1; sq[1, 2] = big; sq[1, 3] = big + 2   # float(big + 1) == float(big): a conversion to double would merge them
    assert float(big + 1) == float(big)
    edges, _ = graph(s, h, sq, knn=3, skip_fixed0=True)
    assert edges == [(1, 2), (1, 0), (1, 3)]
    sq[1, 0] = big - 1
    edges, _ = graph(s, h, sq, knn=2, skip_fixed0=True)
    assert edges == [(1, 0), (1, 2)]
    # equal hits and equal sums: the lower j; and without sums: hits, then the lower j
    sq[1, :] = 7
    assert graph(s, h, sq, knn=2)[0] == [(1, 0), (1, 2)]
    assert graph(s, h, None, knn=3)[0] == [(1, 0), (1, 2), (1, 3)]
    h[1, 3] = 51
    assert graph(s, h, None, knn=2)[0] == [(1, 3), (1, 0)]


def test_min_fraction_and_zero_hit_candidates_are_dropped():
    s = np.array([100, 100, 100], dtype=np.int32)
    h = np.array([[100, 40, 0], [40, 100, 9], [0, 10, 100]], dtype=np.int32)
    edges, nc = graph(s, h, knn=2, min_fraction=0.0, skip_fixed0=False)
    assert edges == [(0, 1), (1, 0), (1, 2), (2, 1)] and nc == 1      # zero hits never make an edge: fewer than knn
    edges, nc = graph(s, h, knn=2, min_fraction=0.1, skip_fixed0=False)
    assert edges == [(0, 1), (1, 0), (2, 1)] and nc == 1              # 9 < 0.1 * 100 <= 10
    edges, nc = graph(s, h, knn=2, min_fraction=0.5, skip_fixed0=False)
    assert edges == [] and nc == 3                                    # a frame may end with no edge at all
    # the fraction refers to the SOURCE frame's samples
    s2 = np.array([100, 100, 20], dtype=np.int32)
    assert graph(s2, h, knn=2, min_fraction=0.5, skip_fixed0=False)[0] == [(2, 1)]


def test_knn_at_least_K_keeps_every_candidate():
    s, h = chain_table(4)
    for knn in (3, 4, 50):
        edges, nc = graph(s, h, knn=knn, skip_fixed0=False, cap=12)
        assert edges == [(0, 1), (0, 2), (1, 0), (1, 2), (1, 3), (2, 1), (2, 3), (2, 0), (3, 2), (3, 1)] and nc == 1
    assert graph(s, h, knn=50, skip_fixed0=False)[0] == edges           # the default capacity is K * min(knn, K - 1)
    assert graph(s, h, knn=0)[0] == []


def test_cap_too_small_is_an_error_with_a_message():
    s, h = chain_table(4)
    with pytest.raises(mvicp.MvicpError, match="more than cap = 3 edges"):
        mvicp.graph_from_overlap(s, h, knn=2, skip_fixed0=False, cap=3)
    src, dst, _ = mvicp.graph_from_overlap(s, h, knn=2, skip_fixed0=True, cap=6)   # exactly enough
    assert len(src) == 6


def test_components():
    s, h = chain_table(6)
    assert graph(s, h, knn=2)[1] == 1
    # two islands {0,1,2} and {3,4,5}
    h2 = h.copy()
    h2[:3, 3:] = 0; h2[3:, :3] = 0
    edges, nc = graph(s, h2, knn=2)
    assert nc == 2 and all((a < 3) == (b < 3) for a, b in edges)
    # an island that is only reachable through an edge OUT OF frame 0: {1, 2} never name frame 0, frame 0 names 1
    s3 = np.full(3, 10, dtype=np.int32)
    h3 = np.array([[10, 5, 0], [0, 10, 5], [0, 5, 10]], dtype=np.int32)
    edges, nc = graph(s3, h3, knn=1, skip_fixed0=True)
    assert edges == [(1, 2), (2, 1)] and nc == 1
    edges, nc = graph(s3, h3, knn=1, skip_fixed0=False)
    assert edges == [(0, 1), (1, 2), (2, 1)] and nc == 1
    h3[0, 1] = 0
    assert graph(s3, h3, knn=1)[1] == 2
    assert graph(np.zeros(0, np.int32), np.zeros((0, 0), np.int32))[1] == 0


@pytest.mark.parametrize("n,ms", [(20000, 0), (20000, -3), (20000, 20000), (20000, 20001), (20000, 1500), (1, 4096), (1, 0), (7, 3), (1500000000, 4096)])
def test_overlap_sample_indices(n, ms):
    idx = mvicp.overlap_sample_indices(n, ms)   # (the last case needs the 64-bit product: 4095 * 1.5e9 > 2^32)
    s = n if ms <= 0 or ms >= n else ms
    assert idx.dtype == np.int64 and len(idx) == s and idx[0] == 0
    assert np.array_equal(idx, (np.arange(s, dtype=np.int64) * n) // s)
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    if s == n:
        assert np.array_equal(idx, np.arange(n))


def test_overlap_sample_indices_empty():
    assert len(mvicp.overlap_sample_indices(0, 4096)) == 0 and len(mvicp.overlap_sample_indices(0, 0)) == 0


def test_overlap_null_context_is_err_arg(engine_lib):
    P = np.eye(4).reshape(1, 16).copy()
    samples = np.zeros(1, dtype=np.int32); hits = np.zeros(1, dtype=np.int32)
    st = engine_lib.mvicp_overlap(None, P.ctypes.data_as(C.POINTER(C.c_double)), C.c_float(0.05), 0,
                                  samples.ctypes.data_as(C.POINTER(C.c_int)), hits.ctypes.data_as(C.POINTER(C.c_int)), None, None)
    assert st == -1 and b"null context" in engine_lib.mvicp_last_error()
    assert "mvicp_overlap" in L.SYMBOLS and "mvicp_graph_from_overlap" in L.SYMBOLS
