"""-m gpu: mvicp_normal_agreement counts what numpy counts (tests/orientref.py agreement) over searched lists, explicit lists, with a
fixed source and on dots that are exactly 0; mvicp_negate_normals swaps the two counts and, applied twice, restores the bytes; a
registration after mvicp.orient_frames is the registration of an engine uploaded with the normals it leaves."""
import ctypes as C
import functools

import numpy as np
import pytest

import mvicp
import orientref as oref
from mvicp import lib as L
from mvicp import synth
from mvicp.lib import METRIC_SYMMETRIC, MvicpError

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def world():
    """-> (problem of three clouds of 1500 points, its normals with a third of the signs of cloud 1 and all of cloud 2 turned)"""
    pb = synth.make_problem(3, 1500)
    rng = np.random.default_rng(11)
    nor = [np.ascontiguousarray(n).copy() for n in pb["nor"]]
    nor[1][rng.random(len(nor[1])) < 1 / 3] *= -1.0
    nor[2] *= -1.0
    return pb, nor


@pytest.fixture()
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def numpy_counts(e, pb, nor, poses, skip=()):
    pos, neg = [], []
    for k, (s, d) in enumerate(zip(pb["src"], pb["dst"])):
        if k in skip:
            pos.append(0); neg.append(0)
            continue
        f, sec, _ = e.get_correspondences(k)
        a, b = oref.agreement(poses[s], nor[s], f, poses[d], nor[d], sec)
        pos.append(a); neg.append(b)
    return np.array(pos, dtype=np.int32), np.array(neg, dtype=np.int32)


def snor(e, i):
    return e.get_structure(i, "snor").view(np.float64).reshape(-1, 3)[e.get_structure(i, "inv").view(np.int32)]


def test_searched_lists_a_fixed_source_and_negation(eng):
    pb, nor = world()
    eng.set_frames(pb["pts"], nor); eng.set_graph(pb["src"], pb["dst"])
    free = np.zeros(3, dtype=np.uint8)
    counts, _ = eng.correspond(pb["init"], free, 0.05)
    assert (np.asarray(counts) > 300).all()
    blocks = np.asarray(eng.linearize_metric(pb["init"], METRIC_SYMMETRIC, True)).tobytes()
    pos, neg = eng.normal_agreement(pb["init"])
    wp, wn = numpy_counts(eng, pb, nor, pb["init"])
    print("agreement per edge: pos", pos.tolist(), "neg", neg.tolist(), "of", np.asarray(counts).tolist())
    assert pos.tobytes() == wp.tobytes() and neg.tobytes() == wn.tobytes()
    assert (pos > 0).all() and (neg > 0).all() and ((pos + neg) == np.asarray(counts)).all()
    # at other poses the same lists give other rotations (the counts of a rigid scene stay close, the call must read THESE poses)
    turned = pb["init"].copy(); turned[1, :3, :3] = turned[1, :3, :3] @ synth.so3_exp(np.array([0.0, 0.0, np.pi]))
    p2, n2 = eng.normal_agreement(turned)
    w2 = numpy_counts(eng, pb, nor, turned)
    assert p2.tobytes() == w2[0].tobytes() and n2.tobytes() == w2[1].tobytes() and p2.tobytes() != pos.tobytes()
    # history-neutral: the evaluation is what it was, a NULL count is skipped
    assert np.asarray(eng.linearize_metric(pb["init"], METRIC_SYMMETRIC, True)).tobytes() == blocks
    only = np.zeros(eng.E, dtype=np.int32)
    assert eng.lib.mvicp_normal_agreement(eng.h, L._dp(L.poses_to_c(pb["init"])), None, L._ip(only)) == 0 and only.tobytes() == neg.tobytes()
    # negation of frame 1 swaps the counts of every edge that touches it and of no other; twice restores the bytes
    before = [snor(eng, i).tobytes() for i in range(3)]
    eng.negate_normals(1)
    assert snor(eng, 1).tobytes() == (-nor[1]).tobytes() and snor(eng, 0).tobytes() == before[0]
    p3, n3 = eng.normal_agreement(pb["init"])
    touch = (np.asarray(pb["src"]) == 1) | (np.asarray(pb["dst"]) == 1)
    assert touch.any() and not touch.all()
    assert (p3 == np.where(touch, neg, pos)).all() and (n3 == np.where(touch, pos, neg)).all()
    eng.negate_normals(1)
    assert [snor(eng, i).tobytes() for i in range(3)] == before
    p4, n4 = eng.normal_agreement(pb["init"])
    assert p4.tobytes() == pos.tobytes() and n4.tobytes() == neg.tobytes()
    assert np.asarray(eng.linearize_metric(pb["init"], METRIC_SYMMETRIC, True)).tobytes() == blocks
    # a fixed source: its edges hold no list and count nothing, also when an explicit list is installed on one afterwards
    fixed = np.array([0, 1, 0], dtype=np.uint8)
    eng.correspond(pb["init"], fixed, 0.05)
    out0 = [k for k, s in enumerate(pb["src"]) if s == 1]
    assert out0
    p5, n5 = eng.normal_agreement(pb["init"])
    w5 = numpy_counts(eng, pb, nor, pb["init"], skip=out0)
    assert p5.tobytes() == w5[0].tobytes() and n5.tobytes() == w5[1].tobytes() and not p5[out0].any() and not n5[out0].any() and p5.sum() > 0
    ids = np.arange(100, dtype=np.int32)
    eng.set_correspondences(out0[0], ids, ids, 0.05)
    p6, n6 = eng.normal_agreement(pb["init"])
    assert p6.tobytes() == p5.tobytes() and n6.tobytes() == n5.tobytes()


def test_explicit_lists_and_dots_that_are_exactly_zero(eng):
    pb, nor = world()
    rng = np.random.default_rng(5)
    eng.set_frames(pb["pts"], nor); eng.set_graph(pb["src"], pb["dst"])
    lists = {}
    for k, (s, d) in enumerate(zip(pb["src"], pb["dst"])):
        m = int(rng.integers(0, 1200)) if k else 0                       # (edge 0 stays empty; repeats and any order are allowed)
        lists[k] = (rng.integers(0, 1500, m).astype(np.int32), rng.integers(0, 1500, m).astype(np.int32))
        eng.set_correspondences(k, lists[k][0], lists[k][1], 0.05)
    pos, neg = eng.normal_agreement(pb["init"])
    for k, (s, d) in enumerate(zip(pb["src"], pb["dst"])):
        assert (int(pos[k]), int(neg[k])) == oref.agreement(pb["init"][s], nor[s], lists[k][0], pb["init"][d], nor[d], lists[k][1]), k
    assert pos[0] == 0 and neg[0] == 0 and pos[1:].sum() > 0
    # normals along x against normals along y at axis-aligned poses: every dot is exactly 0 and counts on neither side
    n = 700
    p = rng.normal(0, 0.2, (n, 3))
    e2 = mvicp.Engine(0)
    try:
        e2.set_frames([p, p], [np.tile([1.0, 0.0, 0.0], (n, 1)), np.tile([0.0, -1.0, 0.0], (n, 1))]); e2.set_graph([1, 0], [0, 1])
        ids = np.arange(n, dtype=np.int32)
        e2.set_correspondences(0, ids, ids, 0.05); e2.set_correspondences(1, ids[:300], ids[:300], 0.05)
        I = np.array([np.eye(4), np.eye(4)])
        assert [a.tolist() for a in e2.normal_agreement(I)] == [[0, 0], [0, 0]]
        quarter = I.copy(); quarter[1, :3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]   # frame 1 turned by 90 degrees: -y -> +x
        assert [a.tolist() for a in e2.normal_agreement(quarter)] == [[n, 300], [0, 0]]
    finally:
        e2.close()


def test_refusals(eng):
    pb, nor = world()
    P = L._dp(L.poses_to_c(pb["init"]))
    out = np.zeros(8, dtype=np.int32)
    call = lambda: eng.lib.mvicp_normal_agreement(eng.h, P, L._ip(out), L._ip(out[4:]))
    eng.set_frames(pb["pts"], [nor[0], None, nor[2]])
    assert call() == -3                                                   # no graph
    eng.set_graph(pb["src"], pb["dst"])
    assert call() == -3                                                   # no list
    eng.correspond(pb["init"], pb["fixed"], 0.05)
    assert call() == -3 and b"normals on frame 1" in eng.lib.mvicp_last_error()
    assert eng.lib.mvicp_normal_agreement(eng.h, None, L._ip(out), L._ip(out[4:])) == -1
    assert eng.lib.mvicp_negate_normals(eng.h, 1) == -3 and eng.lib.mvicp_negate_normals(eng.h, 3) == -1 and eng.lib.mvicp_negate_normals(eng.h, -1) == -1
    assert snor(eng, 0).tobytes() == nor[0].tobytes()


def test_a_registration_after_orient_frames_is_an_ordinary_one():
    pb, _ = world()
    good = [np.ascontiguousarray(n) for n in pb["nor"]]
    turned = [good[0], -good[1], good[2]]
    fixed = np.asarray(pb["fixed"], dtype=np.uint8)

    def rounds(e):
        P, out = pb["init"].copy(), []
        for _ in range(3):
            c, w = e.correspond(P, fixed, 0.05)
            P, sm = e.optimize_metric(P, fixed, L.PARAM_SOPHUS_SE3, METRIC_SYMMETRIC, True, 50)
            out.append((np.asarray(c).tobytes(), np.asarray(w).tobytes(), P.tobytes(), sm["iterations"], sm["final_cost"]))
        return out

    a, b = mvicp.Engine(0), mvicp.Engine(0)
    try:
        a.set_frames(pb["pts"], turned); a.set_graph(pb["src"], pb["dst"])
        res = mvicp.orient_frames(a, pb["init"], fixed, 0.05, 10)
        assert res["components"] == 1 and res["flip"].tolist() == [0, 1, 0]
        for i in range(3):
            assert snor(a, i).tobytes() == good[i].tobytes()
        b.set_frames(pb["pts"], good); b.set_graph(pb["src"], pb["dst"])
        assert rounds(a) == rounds(b)
    finally:
        a.close(); b.close()
