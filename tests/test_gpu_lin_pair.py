"""-m gpu: the paired evaluation (mvicp_linearize_pair: two pose sets, ONE pass over the operand stream) against two single evaluations.
Bar: byte for byte — the paired kernel evaluates, per pose set, exactly the expressions of the one-pose kernel in the same order, and each
set's partials are summed in the same fixed order.  The round-level switch (option lin_pair) must leave a whole trajectory what it was."""
import numpy as np
import pytest

import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu

FLAGS = [(1, 1), (1, 0), (0, 1), (0, 0)]   # (point_to_plane, robust): every combination has a two-pose build (no spills)


def _second_poses(poses, seed=11, sigma=2e-3, sigmat=1e-3):
    """A second pose set a small step away from the first, like an LM candidate (every view moved, view 0 included)."""
    rng = np.random.default_rng(seed)
    return np.array([synth.add_noise(P, sigma, sigmat, rng) for P in poses])


def _assert_pair_is_two_singles(eng, Pa, Pb, plane, robust):
    ra = eng.linearize(Pa, plane, robust)
    rb = eng.linearize(Pb, plane, robust)
    pa, pb = eng.linearize_pair(Pa, Pb, plane, robust)
    assert np.all(np.isfinite(ra)) and np.all(np.isfinite(rb))
    assert pa.tobytes() == ra.tobytes(), (plane, robust, "first set", float(np.abs(pa - ra).max()))
    assert pb.tobytes() == rb.tobytes(), (plane, robust, "second set", float(np.abs(pb - rb).max()))
    return ra, rb


@pytest.mark.parametrize("plane,robust", FLAGS)
def test_pair_equals_two_single_evaluations_after_a_search(plane, robust):
    """(a) 4 x 4000, lists as one search left them (mostly identity lists: the shared-source-cloud path of the kernel)."""
    pb = synth.make_problem(4, 4000)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
        c, _ = eng.correspond(pb["init"], pb["fixed"], 0.05)
        assert c.sum() > 0
        ra, rb = _assert_pair_is_two_singles(eng, pb["init"], _second_poses(pb["init"]), plane, robust)
        assert ra.tobytes() != rb.tobytes()   # the two pose sets really differ
    finally:
        eng.close()


@pytest.mark.parametrize("plane,robust", FLAGS)
def test_pair_equals_two_single_evaluations_with_rejected_queries(plane, robust):
    """(b) partial overlap (20-degree views, 5 mm cutoff): some queries are rejected, so the lists are not the identity and every edge reads
    its private copy of the source points from the stream."""
    pb = synth.make_problem(4, 4000, cone_deg=20.0, sigma=0.004, sigmat=0.002)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
        c, _ = eng.correspond(pb["init"], pb["fixed"], 0.005)
        n_src = np.array([len(pb["pts"][s]) for s in pb["src"]])
        assert 0 < c.sum() < n_src.sum(), (c, n_src)                 # some, but not all, queries accepted
        assert np.any((c > 0) & (c < n_src)), (c, n_src)             # ... within one edge: a list that is not the identity
        _assert_pair_is_two_singles(eng, pb["init"], _second_poses(pb["init"], sigma=5e-4, sigmat=2e-4), plane, robust)
    finally:
        eng.close()


@pytest.mark.parametrize("plane,robust", FLAGS)
def test_pair_equals_two_single_evaluations_on_odd_and_empty_edges(plane, robust):
    """(c) an edge without correspondences, an odd count that is no multiple of the workgroup chunk (a tail pair with one live lane half),
    and a single correspondence; (d) the same pose set twice."""
    pb = synth.make_problem(4, 4000)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
        c, _ = eng.correspond(pb["init"], pb["fixed"], 0.05)
        rng = np.random.default_rng(3)
        none = np.zeros(0, dtype=np.int32)
        eng.set_correspondences(0, none, none, 0.01)
        n1 = 1237   # odd; 1237 = 2 * 512 + 213: neither a multiple of 2 nor of any chunk size the library picks (512 ... 8192)
        eng.set_correspondences(1, rng.integers(0, 4000, n1).astype(np.int32), rng.integers(0, 4000, n1).astype(np.int32), 0.01)
        eng.set_correspondences(2, np.array([17], dtype=np.int32), np.array([2900], dtype=np.int32), 0.01)
        Pb = _second_poses(pb["init"])
        ra, _ = _assert_pair_is_two_singles(eng, pb["init"], Pb, plane, robust)
        assert not ra[0].any()                                      # the empty edge contributes nothing
        qa, qb = eng.linearize_pair(Pb, Pb, plane, robust)          # (d)
        assert qa.tobytes() == qb.tobytes() == eng.linearize(Pb, plane, robust).tobytes()
    finally:
        eng.close()


def test_pair_leaves_the_queued_evaluations_alone():
    """mvicp_linearize_pair between a search and its solve: the solve still finds its queued first evaluation and ends where it ends without the call."""
    pb = synth.make_problem(4, 4000)
    out = {}
    for probe in (0, 1):
        eng = mvicp.Engine(0)
        try:
            eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
            eng.profile(True)
            poses = pb["init"].copy()
            hits = []
            for r in range(4):
                eng.profile_reset()
                eng.correspond(poses, pb["fixed"], 0.05)
                if probe:
                    eng.linearize_pair(pb["gt"], pb["init"], 1, 1)
                poses, sm = eng.optimize(poses, pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)
                hits.append((eng.profile_get("spec.hit")[1], sm["iterations"], sm["evaluations"]))
            out[probe] = (poses, hits)
        finally:
            eng.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1] and sum(h[0] for h in out[1][1]) >= 2, out


def test_fixed_point_rounds_use_one_paired_launch_and_the_trajectory_is_unchanged():
    """16 rounds as in test_second_queued_evaluation_at_the_fixed_point_is_used_and_exact, with lin_pair = 1 and 0: counts, weights, poses, LM iterations /
    evaluations / termination and the queued-evaluation hits identical round by round; with lin_pair = 1 every round whose second queued evaluation was used
    launched the paired kernel once and the one-pose kernel not at all."""
    pb = synth.make_problem(4, 4000)
    res = {}
    for pair in (1, 0):
        e = mvicp.Engine(0)
        try:
            e.set_option("lin_pair", pair)
            e.set_frames(pb["pts"], pb["nor"]); e.set_graph(pb["src"], pb["dst"])
            e.profile(True)
            poses = pb["init"].copy()
            log = []
            for r in range(16):
                e.profile_reset()
                c, w = e.correspond(poses, pb["fixed"], 0.05)
                param, plane = (L.PARAM_ANGLE_AXIS, 0) if r == 14 else (L.PARAM_SOPHUS_SE3, 1)   # round 14 changes the flags at the fixed point
                poses, sm = e.optimize(poses, pb["fixed"], param, plane, True, 50)
                log.append((c.copy(), w.tobytes(), poses.copy(), sm["iterations"], sm["evaluations"], sm["termination"],
                            e.profile_get("spec.hit")[1], e.profile_get("spec2.hit")[1], e.profile_get("linearize_pair")[1], e.profile_get("linearize")[1]))
            res[pair] = log
        finally:
            e.close()
    for r, (a, b) in enumerate(zip(res[1], res[0])):
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], r
        assert a[2].tobytes() == b[2].tobytes(), r
        assert a[3:8] == b[3:8], (r, a[3:8], b[3:8])
    assert all(l[8] == 0 for l in res[0])                     # lin_pair = 0: the paired kernel is never launched
    h2 = [l[7] for l in res[1]]
    assert sum(h2) >= 4, h2
    for r, l in enumerate(res[1]):
        if l[7] == 1:
            assert l[8] == 1 and l[9] == 0, (r, l[6:])        # both evaluations of the round came from ONE paired launch
            assert res[0][r][9] == 2 and res[0][r][8] == 0, (r, res[0][r][6:])   # ... where lin_pair = 0 launched the one-pose kernel twice
