"""-m gpu: the calls that name the objective — mvicp_linearize_metric, mvicp_optimize_metric (include/mvicp.h).

  * metric 0 / 1 through the new calls ARE the old calls: a 6-round registration driven through them is byte-equal, round by round, to a
    second engine driven through mvicp_linearize / mvicp_optimize, including the number of evaluations served by the queued launch;
  * what the new calls refuse, and that a refusal changes nothing;
  * a symmetric solve queues nothing for the next search, and a plane solve after it arms the queue again;
  * mvicp_optimize_metric(SYMMETRIC) against mvicp_lm_solve over the fp64 rows of tests/symref.py on the same lists;
  * end to end: 25 rounds of search + solve on the two fixtures of tests/test_sym_cpu.py, with either objective."""
import numpy as np
import pytest

import matchref
import mvicp
import symref
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu
ARG, STATE = -1, -3
CUTOFF = 0.05


@pytest.fixture(scope="module")
def pb():
    return synth.make_problem(3, 2000)


def _engine(pb, nor="all"):
    eng = mvicp.Engine(0)
    normals = pb["nor"] if nor == "all" else [None if k in nor else pb["nor"][k] for k in range(len(pb["pts"]))]
    eng.set_frames(pb["pts"], normals)
    eng.set_graph(pb["src"], pb["dst"])
    return eng


@pytest.mark.parametrize("metric", [L.METRIC_PLANE, L.METRIC_POINT])
def test_metric_point_and_plane_are_the_old_calls_byte_for_byte(pb, metric):
    old, new = _engine(pb), _engine(pb)
    try:
        old.profile(1); new.profile(1)
        Po, Pn = pb["init"].copy(), pb["init"].copy()
        for rnd in range(6):
            co, wo = old.correspond(Po, pb["fixed"], CUTOFF)
            cn, wn = new.correspond(Pn, pb["fixed"], CUTOFF)
            assert np.array_equal(co, cn) and wo.tobytes() == wn.tobytes(), rnd
            Po, so = old.optimize(Po, pb["fixed"], L.PARAM_SOPHUS_SE3, metric, True, 50)
            Pn, sn = new.optimize_metric(Pn, pb["fixed"], L.PARAM_SOPHUS_SE3, metric, True, 50)
            assert Po.tobytes() == Pn.tobytes(), rnd
            assert so == sn, (rnd, so, sn)
            bo, bn = old.linearize(Po, metric, True), new.linearize_metric(Pn, metric, True)
            assert bo.tobytes() == bn.tobytes(), rnd
        ho, hn = old.profile_get("spec.hit")[1], new.profile_get("spec.hit")[1]
        print("metric %d: spec.hit old %d new %d" % (metric, ho, hn))
        assert ho == hn and ho >= 1   # (later rounds start from a queued evaluation)
    finally:
        old.close(); new.close()


def _status(eng, name, *args):
    st = int(getattr(eng.lib, name)(eng.h, *args))
    return st, eng.lib.mvicp_last_error().decode()


def _lin_metric_status(eng, poses, metric, out, null_poses=False, null_out=False):
    P = L.poses_to_c(poses)
    return _status(eng, "mvicp_linearize_metric", None if null_poses else L._dp(P), metric, 1, None if null_out else L._dp(out))


def test_what_the_metric_calls_refuse_and_that_a_refusal_changes_nothing(pb):
    """metric 3 / -1 and NULL pointers -> MVICP_ERR_ARG; no list yet, a source or a destination without normals -> MVICP_ERR_STATE naming the
    frame.  After each refusal `out` still holds its sentinel and a plane evaluation returns the bytes it returned before."""
    poses = pb["init"]
    sentinel = np.full((len(pb["src"]), L.EDGE_BLOCK), -7.25)

    def refused(eng, want, fragment, before, **kw):
        out = sentinel.copy()
        st, msg = _lin_metric_status(eng, poses, kw.pop("metric", L.METRIC_SYMMETRIC), out, **kw)
        assert st == want and fragment in msg, (want, fragment, st, msg)
        assert out.tobytes() == sentinel.tobytes()
        if before is not None:
            assert eng.linearize(poses, before[0], True).tobytes() == before[1].tobytes()

    eng = _engine(pb)
    try:
        refused(eng, STATE, "no correspondences", None)                       # no list yet
        with pytest.raises(mvicp.lib.MvicpError, match="no correspondences"):
            eng.optimize_metric(poses, pb["fixed"], L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 5)
        eng.correspond(poses, pb["fixed"], CUTOFF)
        plane = (1, eng.linearize(poses, 1, True))
        refused(eng, ARG, "not an mvicp_metric", plane, metric=3)
        refused(eng, ARG, "not an mvicp_metric", plane, metric=-1)
        refused(eng, ARG, "null", plane, null_poses=True)
        refused(eng, ARG, "null", plane, null_out=True)
        for bad in (3, -1):
            b = eng._round_buffers(len(poses))
            st, msg = _status(eng, "mvicp_optimize_metric", b["pP"], b["pfx"], L.PARAM_SOPHUS_SE3, bad, 1, 5, b["psm"])
            assert st == ARG and "not an mvicp_metric" in msg, (st, msg)
            assert eng.linearize(poses, 1, True).tobytes() == plane[1].tobytes()
        assert np.all(np.isfinite(eng.linearize_metric(poses, L.METRIC_SYMMETRIC, True)))   # (and the call itself works on this engine)
        assert eng.linearize(poses, 1, True).tobytes() == plane[1].tobytes()
    finally:
        eng.close()

    # frame 2 is a source only of its own edges and a destination of others: without its normals both roles are refused, naming frame 2
    srcs, dsts = list(pb["src"]), list(pb["dst"])
    assert 2 in srcs and 2 in dsts
    eng = _engine(pb, nor={2})
    try:
        eng.correspond(poses, pb["fixed"], CUTOFF)
        point = (0, eng.linearize(poses, 0, True))
        refused(eng, STATE, "symmetric needs normals on frame 2", point)
    finally:
        eng.close()
    # source without normals only: a two-frame graph 1 -> 0 where frame 1 (the source) has none; then the destination
    for missing in (1, 0):
        eng = mvicp.Engine(0)
        try:
            eng.set_frames(pb["pts"][:2], [None if k == missing else pb["nor"][k] for k in range(2)])
            eng.set_graph([1], [0])
            eng.correspond(poses[:2], [1, 0], CUTOFF)
            out = np.full((1, L.EDGE_BLOCK), -7.25)
            before = eng.linearize(poses[:2], 0, True)
            st, msg = _lin_metric_status(eng, poses[:2], L.METRIC_SYMMETRIC, out)
            assert st == STATE and "symmetric needs normals on frame %d" % missing in msg, (missing, st, msg)
            assert np.all(out == -7.25)
            assert eng.linearize(poses[:2], 0, True).tobytes() == before.tobytes()
        finally:
            eng.close()


def test_old_calls_with_a_flag_of_two_are_plane_even_when_the_source_has_no_normals(pb):
    """Any non-zero point_to_plane of mvicp_linearize, mvicp_linearize_pair and mvicp_optimize is PLANE, 2 included: never read as
    MVICP_METRIC_SYMMETRIC.  Two frames, the source (frame 1) without normals: the symmetric metric is refused there, flag 2 through the old
    calls returns the bytes of flag 1."""
    poses = pb["init"][:2]
    P2 = np.array([synth.add_noise(P, 2e-3, 1e-3, np.random.default_rng(5)) for P in poses])
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"][:2], [pb["nor"][0], None])
        eng.set_graph([1], [0])
        eng.correspond(poses, [1, 0], CUTOFF)
        with pytest.raises(mvicp.lib.MvicpError, match="symmetric needs normals on frame 1"):
            eng.linearize_metric(poses, L.METRIC_SYMMETRIC, True)
        one = eng.linearize(poses, 1, True)
        assert eng.linearize(poses, 2, True).tobytes() == one.tobytes()
        a1, b1 = eng.linearize_pair(poses, P2, 1, True)
        a2, b2 = eng.linearize_pair(poses, P2, 2, True)
        assert a2.tobytes() == a1.tobytes() == one.tobytes() and b2.tobytes() == b1.tobytes()
        Q1, s1 = eng.optimize(poses, [1, 0], L.PARAM_SOPHUS_SE3, 1, True, 50)
        eng.reset_history()
        eng.correspond(poses, [1, 0], CUTOFF)
        Q2, s2 = eng.optimize(poses, [1, 0], L.PARAM_SOPHUS_SE3, 2, True, 50)
        assert Q2.tobytes() == Q1.tobytes() and s1 == s2, (s1, s2)
    finally:
        eng.close()


def test_nothing_is_queued_after_a_symmetric_solve_and_a_plane_solve_arms_the_queue_again(pb):
    """After a symmetric solve the next search queues no evaluation: spec.hit does not rise in the next round, and the search's counts, weights
    and lists equal those of an engine that only searched at the same poses.  A plane solve after that arms the queue again."""
    eng, ref = _engine(pb), _engine(pb)
    try:
        eng.profile(1)
        P = pb["init"].copy()
        for _ in range(2):                                   # two plane rounds: the second starts from a queued evaluation
            eng.correspond(P, pb["fixed"], CUTOFF)
            P, _ = eng.optimize(P, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
        hits = eng.profile_get("spec.hit")[1]
        assert hits >= 1
        eng.correspond(P, pb["fixed"], CUTOFF)               # (queues a plane evaluation, which the symmetric solve must not use)
        P, sm = eng.optimize_metric(P, pb["fixed"], L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
        assert eng.profile_get("spec.hit")[1] == hits and sm["evaluations"] >= 1
        c, w = eng.correspond(P, pb["fixed"], CUTOFF)        # the search after the symmetric solve
        cr, wr = ref.correspond(P, pb["fixed"], CUTOFF)
        assert np.array_equal(c, cr) and w.tobytes() == wr.tobytes()
        for e in range(len(pb["src"])):
            for a, b in zip(eng.get_correspondences(e), ref.get_correspondences(e)):
                assert a.tobytes() == b.tobytes(), e
        P2, _ = eng.optimize_metric(P, pb["fixed"], L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
        assert eng.profile_get("spec.hit")[1] == hits        # nothing was queued, so nothing was served
        eng.correspond(P2, pb["fixed"], CUTOFF)
        P3, _ = eng.optimize(P2, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)    # a plane solve: not served (nothing queued), but it arms
        assert eng.profile_get("spec.hit")[1] == hits
        eng.correspond(P3, pb["fixed"], CUTOFF)
        eng.optimize(P3, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
        assert eng.profile_get("spec.hit")[1] == hits + 1    # the queue is armed again
    finally:
        eng.close(); ref.close()


def _pair_engine(cl):
    eng = mvicp.Engine(0)
    eng.set_frames([cl["dst"], cl["src"]], [cl["dst_nrm"], cl["src_nrm"]])
    eng.set_graph([1], [0])
    return eng


def test_symmetric_solve_equals_the_host_solve_over_the_fp64_rows():
    """mvicp_optimize_metric(SYMMETRIC) on the full-overlap pair, lists from one search at the perturbed start, against mvicp_lm_solve over
    symref.blocks_fp64 on the same lists.  Bound: what the suite holds the other objectives to for one solve against the fp64 oracle (DESIGN.md
    section 7: poses 1e-9 after one solve; 1e-7 per round over whole loops), in translation and in rotation."""
    cl = matchref.e2e_clouds(False)
    P0 = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
    eng = _pair_engine(cl)
    try:
        counts, weights = eng.correspond(P0, [1, 0], 3.0 * cl["spacing"])
        first, second, _ = eng.get_correspondences(0)
        assert counts[0] == len(first) > 1000
        P, sm = eng.optimize_metric(P0, [1, 0], L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC, True, 50)
    finally:
        eng.close()
    p, q, nq, npn = cl["src"][first], cl["dst"][second], cl["dst_nrm"][second], cl["src_nrm"][first]
    Ph, smh = L.lm_solve_host(2, [1], [0], P0, [1, 0], L.PARAM_SOPHUS_SE3,
                              lambda poses: symref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], weights[0], True)[None, :], 50)
    dt, dr = synth.pose_diff(P[1], Ph[1])
    print("symmetric solve, device against host fp64 rows: dt %.2e dr %.2e  (iterations %d / %d, final cost %.12e / %.12e)" % (
        dt, dr, sm["iterations"], smh["iterations"], sm["final_cost"], smh["final_cost"]))
    assert P[0].tobytes() == P0[0].tobytes()
    assert dt <= 1e-9 and dr <= 1e-9, (dt, dr)
    assert sm["iterations"] == smh["iterations"]


@pytest.mark.parametrize("partial", [False, True])
def test_symmetric_registration_on_the_gpu_ends_closer_to_the_truth_than_point_to_plane(partial):
    """tests/test_sym_cpu.py's registration through the library: 25 rounds of mvicp_correspond + mvicp_optimize_metric from the truth perturbed
    by 3 degrees and one spacing, cutoff 3 spacings, with PLANE and with SYMMETRIC.  Asserted: the same ordering, in rotation and in the largest
    point displacement.  CPU figures: 0.0315 deg / 0.055 spacings against 0.0045 / 0.0063 (full), 0.082 / 0.109 against 0.0041 / 0.0083 (partial)."""
    cl = matchref.e2e_clouds(partial)
    got = {}
    for metric in (L.METRIC_PLANE, L.METRIC_SYMMETRIC):
        eng = _pair_engine(cl)
        try:
            P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
            for _ in range(25):
                eng.correspond(P, [1, 0], 3.0 * cl["spacing"])
                P, _ = eng.optimize_metric(P, [1, 0], L.PARAM_SOPHUS_SE3, metric, True, 50)
        finally:
            eng.close()
        got[metric] = symref.distance_to_truth(P[1], cl["truth"], cl["src"], cl["spacing"])
    a, b = got[L.METRIC_PLANE], got[L.METRIC_SYMMETRIC]
    print("GPU partial=%s  point-to-plane ends %.4f deg, %.4f spacings  |  symmetric ends %.4f deg, %.4f spacings  (ratios %.1f, %.1f)" % (
        partial, a[0], a[1], b[0], b[1], a[0] / b[0], a[1] / b[1]))
    assert b[0] < a[0] and b[1] < a[1], got
