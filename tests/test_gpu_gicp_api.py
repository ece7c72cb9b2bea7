"""-m gpu: the plane-to-plane (Generalized-ICP) entry points — mvicp_linearize_gicp, mvicp_optimize_gicp (include/mvicp.h).

  * what they refuse (epsilon outside [1e-6, 1], a NaN, NULL pointers, no graph, no lists, a frame without normals), with which status and
    message, and that after each refusal the POINT / PLANE / SYMMETRIC blocks, the lists and the epochs are byte for byte what they were;
  * POINT / PLANE / SYMMETRIC evaluations before and after a GICP evaluation and a GICP solve are byte-identical; the search after a GICP solve
    queues no evaluation; after mvicp_recompute_normals on the source frame the next evaluation sees the new normals;
  * mvicp_optimize_gicp against mvicp_lm_solve over the fp64 rows of tests/gicpref.py on the same lists;
  * end to end: 25 rounds of search + solve on the two fixtures of tests/test_gicp_cpu.py against point-to-plane."""
import ctypes as C

import numpy as np
import pytest

import gicpref
import matchref
import mvicp
import symcases
import symref
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
ARG, STATE = -1, -3
CUTOFF = 0.05
EPS = 1e-3


@pytest.fixture(scope="module")
def pb():
    return synth.make_problem(3, 2000)


def _engine(pb, nor="all"):
    eng = mvicp.Engine(0)
    normals = pb["nor"] if nor == "all" else [None if k in nor else pb["nor"][k] for k in range(len(pb["pts"]))]
    eng.set_frames(pb["pts"], normals)
    eng.set_graph(pb["src"], pb["dst"])
    return eng


def _status(eng, name, *args):
    st = int(getattr(eng.lib, name)(eng.h, *args))
    return st, eng.lib.mvicp_last_error().decode()


def _lin_status(eng, poses, eps, out, null_poses=False, null_out=False):
    P = L.poses_to_c(poses)
    return _status(eng, "mvicp_linearize_gicp", None if null_poses else L._dp(P), C.c_double(eps), 1, None if null_out else L._dp(out))


def _opt_status(eng, poses, fixed, eps):
    """-> (status, message, poses buffer after the call)"""
    b = eng._round_buffers(len(poses))
    np.copyto(b["P44"], np.transpose(np.asarray(poses, dtype=np.float64), (0, 2, 1)))
    b["fx"][:] = fixed
    before = b["P44"].copy()
    st, msg = _status(eng, "mvicp_optimize_gicp", b["pP"], b["pfx"], L.PARAM_SOPHUS_SE3, C.c_double(eps), 1, 5, b["psm"])
    return st, msg, before.tobytes() == b["P44"].tobytes()


def _observables(eng, poses, metrics):
    """what a refused call must leave alone: the blocks of the objectives this engine can evaluate, every list, the epochs"""
    out = [eng.linearize_metric(poses, m, True).tobytes() for m in metrics]
    for e in range(eng.E):
        out += [a.tobytes() for a in eng.get_correspondences(e)]
    out.append(eng.correspondence_epochs().tobytes())
    return out


BAD_EPSILONS = [0.0, 9.99e-7, 1.0000001, 2.0, -1e-3, float("nan"), float("inf"), -float("inf")]


def test_what_the_gicp_calls_refuse_and_that_a_refusal_changes_nothing(pb):
    poses = pb["init"]
    sentinel = np.full((len(pb["src"]), L.EDGE_BLOCK), -7.25)
    all_metrics = (L.METRIC_POINT, L.METRIC_PLANE, L.METRIC_SYMMETRIC)

    def refused_lin(eng, want, fragment, metrics, eps=EPS, **kw):
        before = _observables(eng, poses, metrics) if metrics else None
        out = sentinel.copy()
        st, msg = _lin_status(eng, poses, eps, out, **kw)
        assert st == want and fragment in msg, (want, fragment, st, msg)
        assert out.tobytes() == sentinel.tobytes()
        if metrics:
            assert _observables(eng, poses, metrics) == before, (fragment, eps)

    def refused_opt(eng, want, fragment, metrics, eps=EPS):
        before = _observables(eng, poses, metrics) if metrics else None
        st, msg, same = _opt_status(eng, poses, pb["fixed"], eps)
        assert st == want and fragment in msg and same, (want, fragment, st, msg, same)
        if metrics:
            assert _observables(eng, poses, metrics) == before, (fragment, eps)

    # no graph
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        out = sentinel.copy()
        st, msg = _lin_status(eng, poses, EPS, out)
        assert st == STATE and "no graph" in msg and out.tobytes() == sentinel.tobytes(), (st, msg)
        st, msg, same = _opt_status(eng, poses, pb["fixed"], EPS)
        assert st == STATE and "no graph" in msg and same, (st, msg)
    finally:
        eng.close()

    eng = _engine(pb)
    try:
        refused_lin(eng, STATE, "no correspondences", None)                       # no list yet
        refused_opt(eng, STATE, "no correspondences", None)
        eng.correspond(poses, pb["fixed"], CUTOFF)
        for eps in BAD_EPSILONS:
            refused_lin(eng, ARG, "gicp epsilon", all_metrics, eps=eps)
            refused_opt(eng, ARG, "gicp epsilon", all_metrics, eps=eps)
        refused_lin(eng, ARG, "null", all_metrics, null_poses=True)
        refused_lin(eng, ARG, "null", all_metrics, null_out=True)
        for eps in (1e-6, 1.0):                                                   # the ends of the range are inside it
            assert np.all(np.isfinite(eng.linearize_gicp(poses, eps, True)))
        # the metric calls still refuse 3: the objective has no mvicp_metric value
        with pytest.raises(mvicp.lib.MvicpError, match="not an mvicp_metric"):
            eng.linearize_metric(poses, 3, True)
    finally:
        eng.close()
    st = int(eng.lib.mvicp_linearize_gicp(None, L._dp(L.poses_to_c(poses)), C.c_double(EPS), 1, L._dp(sentinel.copy())))
    assert st == ARG

    # frame 2 is a source of some edges and a destination of others: without its normals both roles are refused, naming frame 2
    assert 2 in list(pb["src"]) and 2 in list(pb["dst"])
    eng = _engine(pb, nor={2})
    try:
        eng.correspond(poses, pb["fixed"], CUTOFF)
        refused_lin(eng, STATE, "gicp needs normals on frame 2", (L.METRIC_POINT,))
        refused_opt(eng, STATE, "gicp needs normals on frame 2", (L.METRIC_POINT,))
    finally:
        eng.close()
    # a two-frame graph 1 -> 0 where the source (frame 1), then the destination (frame 0), has none
    for missing in (1, 0):
        eng = mvicp.Engine(0)
        try:
            eng.set_frames(pb["pts"][:2], [None if k == missing else pb["nor"][k] for k in range(2)])
            eng.set_graph([1], [0])
            eng.correspond(poses[:2], [1, 0], CUTOFF)
            out = np.full((1, L.EDGE_BLOCK), -7.25)
            before = eng.linearize(poses[:2], 0, True)
            st, msg = _lin_status(eng, poses[:2], EPS, out)
            assert st == STATE and "gicp needs normals on frame %d" % missing in msg, (missing, st, msg)
            assert np.all(out == -7.25)
            assert eng.linearize(poses[:2], 0, True).tobytes() == before.tobytes()
        finally:
            eng.close()


def test_other_objectives_are_untouched_by_gicp_calls_and_nothing_is_queued_after_a_gicp_solve(pb):
    """POINT / PLANE / SYMMETRIC blocks at fixed poses on fixed lists before a GICP evaluation, after it, and after a GICP solve: the same bytes.
    After a GICP solve the next search queues no evaluation: spec.hit does not rise in the next round, and the search's counts, weights and
    lists equal those of an engine that only searched at the same poses.  A plane solve after that arms the queue again."""
    eng, ref = _engine(pb), _engine(pb)
    metrics = (L.METRIC_POINT, L.METRIC_PLANE, L.METRIC_SYMMETRIC)
    try:
        eng.profile(1)
        P = pb["init"].copy()
        for _ in range(2):                                   # two plane rounds: the second starts from a queued evaluation
            eng.correspond(P, pb["fixed"], CUTOFF)
            P, _ = eng.optimize(P, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
        hits = eng.profile_get("spec.hit")[1]
        assert hits >= 1
        eng.correspond(P, pb["fixed"], CUTOFF)               # (queues a plane evaluation, which the GICP solve must not use)
        P, sm = eng.optimize_gicp(P, pb["fixed"], L.PARAM_SOPHUS_SE3, EPS, True, 50)
        assert eng.profile_get("spec.hit")[1] == hits and sm["evaluations"] >= 1
        c, w = eng.correspond(P, pb["fixed"], CUTOFF)        # the search after the GICP solve
        cr, wr = ref.correspond(P, pb["fixed"], CUTOFF)
        assert np.array_equal(c, cr) and w.tobytes() == wr.tobytes()
        for e in range(len(pb["src"])):
            for a, b in zip(eng.get_correspondences(e), ref.get_correspondences(e)):
                assert a.tobytes() == b.tobytes(), e
        # on these lists, at poses of their own: the three other objectives before a GICP evaluation, after it, and after a GICP solve
        Q = pb["init"]
        before = [eng.linearize_metric(Q, m, True).tobytes() for m in metrics]
        blk = eng.linearize_gicp(Q, EPS, True)
        assert np.all(np.isfinite(blk)) and blk.tobytes() not in before
        assert [eng.linearize_metric(Q, m, True).tobytes() for m in metrics] == before
        P2, _ = eng.optimize_gicp(P, pb["fixed"], L.PARAM_SOPHUS_SE3, EPS, True, 50)
        assert eng.profile_get("spec.hit")[1] == hits        # nothing was queued, so nothing was served
        assert [eng.linearize_metric(Q, m, True).tobytes() for m in metrics] == before
        assert eng.linearize_gicp(Q, EPS, True).tobytes() == blk.tobytes()
        eng.correspond(P2, pb["fixed"], CUTOFF)
        P3, _ = eng.optimize(P2, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)    # a plane solve: not served (nothing queued), but it arms
        assert eng.profile_get("spec.hit")[1] == hits
        eng.correspond(P3, pb["fixed"], CUTOFF)
        eng.optimize(P3, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
        assert eng.profile_get("spec.hit")[1] == hits + 1    # the queue is armed again
    finally:
        eng.close(); ref.close()


def test_gicp_evaluation_sees_recomputed_source_normals():
    """mvicp_recompute_normals on the SOURCE frame between two evaluations: the first is gicpref's with the uploaded source normals, the second
    with the normals the call returned, each within the accuracy sweep's bar (tests/test_gpu_gicp_accuracy.py)."""
    case = symcases.make_case("recompute", seed=900, N=2001, M=3000, chunk=512)
    eng = mvicp.Engine(0)
    try:
        eng.set_option("lin_chunk", 512)
        eng.set_frames([case["dst"], case["src"]], [case["nor"], case["snor"]])
        eng.set_graph([1], [0])
        eng.set_correspondences(0, case["first"], case["second"], case["a"])

        def check(snor, label):
            p, q, nq, npn = symcases.gathered(dict(case, snor=snor))
            ref = gicpref.edge_block(p, q, nq, npn, case["poses"][1], case["poses"][0], case["a"], EPS, 1)
            err_ref = gicpref.piece_errors(gicpref.unpack(gicpref.blocks_fp64(p, q, nq, npn, case["poses"][1], case["poses"][0], case["a"], EPS, 1)), ref)
            blk = eng.linearize_gicp(case["poses"], EPS, True)[0]
            ratio, where = gicpref.worst_ratio(gicpref.piece_errors(gicpref.unpack(blk), ref), err_ref)
            print("GICP %s: worst ratio %.2f at %s" % (label, ratio, where))
            assert ratio <= 32.0, (label, ratio, where)
            return blk

        b0 = check(case["snor"], "before recompute_normals")
        new = eng.recompute_normals(1, 10)
        assert new.shape == case["snor"].shape and not np.allclose(new, case["snor"])
        b1 = check(new, "after recompute_normals(src)")
        assert b0.tobytes() != b1.tobytes()
    finally:
        eng.close()


def _pair_engine(cl):
    eng = mvicp.Engine(0)
    eng.set_frames([cl["dst"], cl["src"]], [cl["dst_nrm"], cl["src_nrm"]])
    eng.set_graph([1], [0])
    return eng


def test_gicp_solve_equals_the_host_solve_over_the_fp64_rows():
    """mvicp_optimize_gicp on the full-overlap pair, lists from one search at the perturbed start, against mvicp_lm_solve over
    gicpref.blocks_fp64 on the same lists.  Bound: the project's for one solve against fp64 rows: poses within 1e-9 in
    translation and in rotation, and the same number of iterations."""
    cl = matchref.e2e_clouds(False)
    P0 = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
    eng = _pair_engine(cl)
    try:
        counts, weights = eng.correspond(P0, [1, 0], 3.0 * cl["spacing"])
        first, second, _ = eng.get_correspondences(0)
        assert counts[0] == len(first) > 1000
        P, sm = eng.optimize_gicp(P0, [1, 0], L.PARAM_SOPHUS_SE3, EPS, True, 50)
    finally:
        eng.close()
    p, q, nq, npn = cl["src"][first], cl["dst"][second], cl["dst_nrm"][second], cl["src_nrm"][first]
    Ph, smh = L.lm_solve_host(2, [1], [0], P0, [1, 0], L.PARAM_SOPHUS_SE3,
                              lambda poses: gicpref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], weights[0], EPS, True)[None, :], 50)
    dt, dr = synth.pose_diff(P[1], Ph[1])
    print("gicp solve, device against host fp64 rows: dt %.2e dr %.2e  (iterations %d / %d, final cost %.12e / %.12e)" % (
        dt, dr, sm["iterations"], smh["iterations"], sm["final_cost"], smh["final_cost"]))
    assert P[0].tobytes() == P0[0].tobytes()
    assert dt <= 1e-9 and dr <= 1e-9, (dt, dr)
    assert sm["iterations"] == smh["iterations"]


@pytest.mark.parametrize("partial", [False, True])
def test_gicp_registration_on_the_gpu_ends_closer_to_the_truth_than_point_to_plane(partial):
    """tests/test_gicp_cpu.py's registration through the library: 25 rounds of mvicp_correspond + mvicp_optimize_gicp(1e-3) from the truth
    perturbed by 3 degrees and one spacing, cutoff 3 spacings, against mvicp_optimize_metric(PLANE).  Asserted: the same ordering, in rotation
    and in the largest point displacement.  CPU figures: 0.0315 deg / 0.0549 spacings (plane) against 0.0014 / 0.0037 (full),
    0.0817 / 0.1091 against 0.0049 / 0.0098 (partial)."""
    cl = matchref.e2e_clouds(partial)
    got = {}
    for name in ("plane", "gicp"):
        eng = _pair_engine(cl)
        try:
            P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
            for _ in range(25):
                eng.correspond(P, [1, 0], 3.0 * cl["spacing"])
                if name == "gicp":
                    P, _ = eng.optimize_gicp(P, [1, 0], L.PARAM_SOPHUS_SE3, EPS, True, 50)
                else:
                    P, _ = eng.optimize_metric(P, [1, 0], L.PARAM_SOPHUS_SE3, L.METRIC_PLANE, True, 50)
        finally:
            eng.close()
        got[name] = symref.distance_to_truth(P[1], cl["truth"], cl["src"], cl["spacing"])
    a, b = got["plane"], got["gicp"]
    print("GPU partial=%s  point-to-plane ends %.4f deg, %.4f spacings  |  gicp ends %.4f deg, %.4f spacings  (ratios %.1f, %.1f)" % (
        partial, a[0], a[1], b[0], b[1], a[0] / b[0], a[1] / b[1]))
    assert b[0] < a[0] and b[1] < a[1], got


def test_epsilon_belongs_to_the_call_and_is_not_kept(pb):
    """epsilon is an argument of every plane-to-plane call; the context keeps the last one (c->gicp_eps) only for the evaluations of a running
    solve.  On the 3-frame problem: mvicp_linearize_gicp(Q, 1e-3), then mvicp_optimize_gicp at 1e-2, then mvicp_linearize_gicp(Q, 1e-3) again give
    the same bytes; and mvicp_linearize_gicp(Q, 1e-2) after a solve at 1e-3 equals the same call on a fresh engine that holds the same lists."""
    eng, fresh = _engine(pb), _engine(pb)
    try:
        Q = pb["init"]
        c, w = eng.correspond(Q, pb["fixed"], CUTOFF)
        first = eng.linearize_gicp(Q, 1e-3, True)
        P, sm = eng.optimize_gicp(Q, pb["fixed"], L.PARAM_SOPHUS_SE3, 1e-2, True, 50)
        assert sm["successful_steps"] >= 1 and not np.array_equal(P, Q)
        again = eng.linearize_gicp(Q, 1e-3, True)
        assert again.tobytes() == first.tobytes(), float(np.abs(again - first).max())
        eng.optimize_gicp(Q, pb["fixed"], L.PARAM_SOPHUS_SE3, 1e-3, True, 50)
        got = eng.linearize_gicp(Q, 1e-2, True)
        cf, wf = fresh.correspond(Q, pb["fixed"], CUTOFF)        # the same search: the same lists and scales
        assert np.array_equal(c, cf) and w.tobytes() == wf.tobytes()
        for e in range(len(pb["src"])):
            for x, y in zip(eng.get_correspondences(e), fresh.get_correspondences(e)):
                assert x.tobytes() == y.tobytes(), e
        want = fresh.linearize_gicp(Q, 1e-2, True)
        assert got.tobytes() == want.tobytes(), float(np.abs(got - want).max())
        assert got.tobytes() != first.tobytes() and np.all(np.isfinite(got))
    finally:
        eng.close(); fresh.close()
