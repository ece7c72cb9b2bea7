"""-m gpu: Engine.reject_correspondences -- the lists it installs are mvicp.reject_by_mask over the searched lists, byte for byte; an
evaluation over them equals one over the same lists installed on a second engine; and the registration of the partial-overlap pair ends
closer to the truth with target-side rejection than without, as on the CPU (tests/test_boundary_cpu.py)."""
import numpy as np
import pytest

import boundref as br
import matchref
import mvicp
import symref
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu

# tests/test_boundary_cpu.py, partial pair: (deg, spacings) without -> with target-side rejection
CPU = {L.METRIC_PLANE: ((0.0817, 0.1091), (0.0467, 0.0716)), L.METRIC_SYMMETRIC: ((0.0041, 0.0083), (0.0017, 0.0032))}


@pytest.fixture(scope="module")
def world():
    pb = synth.make_problem(4, 3000)
    eng = mvicp.Engine(0)
    eng.set_frames(pb["pts"], pb["nor"])
    masks = [eng.boundary(i, 30)["flag"] for i in range(4)]
    for i in range(4):   # (the masks are the reference's: flagged and unflagged points in every view)
        want = br.boundary(pb["pts"][i], pb["nor"][i], 30, 0.0, -0.5)
        assert masks[i].tobytes() == want["flag"].tobytes() and 0 < want["boundary"] < 3000
    eng.set_graph(pb["src"], pb["dst"])
    yield pb, eng, masks
    eng.close()


@pytest.mark.parametrize("sides", ["dst", "both"])
def test_installed_lists_are_reject_by_mask_over_the_searched_lists(world, sides):
    pb, eng, masks = world
    E = len(pb["src"])
    eng.reset_history()
    counts, weights = eng.correspond(pb["init"], pb["fixed"], 0.05)
    before = [eng.get_correspondences(e) for e in range(E)]
    epochs = eng.correspondence_epochs()
    src_masks = masks if sides == "both" else None
    dropped = eng.reject_correspondences(masks, src_masks)
    assert dropped.dtype == np.int32 and dropped.shape == (E,)
    total = 0
    for e in range(E):
        first, second, dist = before[e]
        assert len(first) == counts[e]
        kf, ks = br.reject_by_mask(first, second, None if src_masks is None else src_masks[pb["src"][e]], masks[pb["dst"][e]])
        gf, gs, gd = eng.get_correspondences(e)
        assert gf.tobytes() == kf.tobytes() and gs.tobytes() == ks.tobytes() and not gd.any() and len(gd) == len(kf)
        assert dropped[e] == len(first) - len(kf)
        total += int(dropped[e])
    assert 0 < total < int(counts.sum())                      # pairs were dropped, and pairs stayed
    assert (eng.correspondence_epochs() != epochs).all()      # every installed list is a new list
    # an evaluation over the installed lists and the searched weights equals one over the same lists on a second engine, byte for byte
    other = mvicp.Engine(0)
    try:
        other.set_frames(pb["pts"], pb["nor"]); other.set_graph(pb["src"], pb["dst"])
        for e in range(E):
            gf, gs, _ = eng.get_correspondences(e)
            other.set_correspondences(e, gf, gs, weights[e])
        for plane in (False, True):
            a, b = np.asarray(eng.linearize(pb["init"], plane, True)), np.asarray(other.linearize(pb["init"], plane, True))
            assert a.tobytes() == b.tobytes() and np.abs(a).sum() > 0
    finally:
        other.close()
    # the next search replaces the explicit lists by searched ones: the counts are the search's again
    counts2, _ = eng.correspond(pb["init"], pb["fixed"], 0.05)
    assert counts2.tobytes() == counts.tobytes()


def test_reject_needs_a_search(world):
    pb, _, masks = world
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"]); eng.set_graph(pb["src"], pb["dst"])
        with pytest.raises(mvicp.MvicpError):
            eng.reject_correspondences(masks)
    finally:
        eng.close()


@pytest.mark.parametrize("metric", [L.METRIC_PLANE, L.METRIC_SYMMETRIC])
def test_registration_of_the_partial_pair_ends_closer_with_target_side_rejection(metric):
    """The 25-round loop of tests/test_gpu_sym_api.py on the partial pair, without and with reject_correspondences(target masks at (30,
    -0.5)) between the search and the solve.  Asserted: the CPU's ordering, in rotation and in the largest point displacement."""
    cl = matchref.e2e_clouds(True)
    got = {}
    for reject in (False, True):
        eng = mvicp.Engine(0)
        try:
            eng.set_frames([cl["dst"], cl["src"]], [cl["dst_nrm"], cl["src_nrm"]])
            mask = eng.boundary(0, 30, 0.0, -0.5)["flag"]
            assert mask.tobytes() == br.boundary(cl["dst"], cl["dst_nrm"], 30, 0.0, -0.5)["flag"].tobytes() and int(mask.sum()) == 131
            eng.set_graph([1], [0])
            P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
            dropped = 0
            for _ in range(25):
                eng.correspond(P, [1, 0], 3.0 * cl["spacing"])
                if reject:
                    dropped += int(eng.reject_correspondences([mask, None])[0])
                P, _ = eng.optimize_metric(P, [1, 0], L.PARAM_SOPHUS_SE3, metric, True, 50)
            assert (dropped > 0) == reject
        finally:
            eng.close()
        got[reject] = symref.distance_to_truth(P[1], cl["truth"], cl["src"], cl["spacing"])
    a, b = got[False], got[True]
    print("GPU partial pair, metric %d: none %.4f deg, %.4f spacings | target-side rejection %.4f deg, %.4f spacings   (CPU: %.4f, %.4f | %.4f, %.4f)" % (
        (metric, a[0], a[1], b[0], b[1]) + CPU[metric][0] + CPU[metric][1]))
    assert b[0] < a[0] and b[1] < a[1], got
