"""-m gpu: the Frame / Session / ICP_Ceres mirror (mv-lm-icp_amd/host/frame.h, the drop-in boundary) driven through
bin/frame_harness.so in call orders, with option switches, cloud changes and failures that bin/multiview never produces.  The mirror is
~500 lines of pointer-keyed caching: a wrong key does not crash, it answers from a cloud that is no longer there with status OK.

Every answer is compared by bytes with a reference that does not go through the mirror (tests/mirrorcases.py): lists, counts and
weights with the CPU oracle at the poses the frames hold; NN answers with the oracle and the real nanoflann; k-NN tables, voxel /
outlier / ISS outputs with the same stage of a fresh mvicp.Engine on the current cloud; poses after a solve with a twin engine driven
with the same searches and solves.  The rule under test is stated in host/frame.h ("WHAT THE MIRROR NOTICES")."""
import numpy as np
import pytest

import framelib
import mirrorcases as mc
import mvicp
from mvicp import lib as L
from mvicp import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pb():
    return synth.make_problem(4, 1500)


@pytest.fixture(scope="module")
def other():
    return synth.make_problem(4, 1200, seed_base=2000)


@pytest.fixture()
def mirror():
    m = framelib.Mirror()
    m.reset_all()        # the session is process-wide: every test starts and ends with Session::reset()
    yield m
    m.reset_all()


# ---------------------------------------------------------------- A: the reference's loop in orders the driver never uses
ORDERS = {
    "forward": [[0, 1, 2, 3]] * 3,
    "reverse": [[3, 2, 1, 0]] * 3,
    "twice": [[0, 0, 1, 1, 2, 2, 3, 3]] * 3,
    "partial": [[1, 3], [0, 1, 2, 3], [0, 1, 2, 3]],
}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_loop_orders(mirror, orc, pb, order):
    """Three rounds of { computeClosestPointsToNeighbours(frame); ceresOptimizer_sophusSE3 } per frame.  After every call the called
    frame holds the oracle's lists and weights and every other frame what it had; copied + skipped accounts for every edge visited; a
    second call in the same round copies nothing; every solve equals the twin's (a solve before any search is refused by both)."""
    M = mc.Model(mirror, orc, pb)
    searched = False
    for rnd in ORDERS[order]:
        for i in rnd:
            M.search(i)
            if not mirror.get_fixed(M.slots[i]):
                searched = True
                copied, skipped = M.search(i)
                assert (copied, skipped) == (0, len(M.expect[M.slots[i]])), (order, i, copied, skipped)
            assert (M.solve() is None) == searched   # (only a solve before the first search is refused: "no correspondences")
    assert searched
    M.close()


# ---------------------------------------------------------------- B: switches at unchanged poses
def test_copy_back_switched_on_at_unchanged_poses(mirror, orc, pb):
    """copy_back false -> search -> true -> the same call again, nothing else changed: the lists are the oracle's (not empty)."""
    M = mc.Model(mirror, orc, pb)
    mirror.set_option(framelib.OPT_COPY_BACK, 0); M.copy_back = False
    for i in range(4):
        M.search(i)                      # weights set, lists empty
    mirror.set_option(framelib.OPT_COPY_BACK, 1); M.copy_back = True
    for i in range(4):
        M.search(i)
        assert i == 0 or all(len(t) > 0 for _, _, t in M.expect[M.slots[i]])
    assert M.solve() is None
    M.close()


def test_copy_back_on_off_on(mirror, orc, pb):
    M = mc.Model(mirror, orc, pb)
    for on in (1, 0, 1):
        mirror.set_option(framelib.OPT_COPY_BACK, on); M.copy_back = bool(on)
        for i in (2, 1, 3):
            M.search(i)
    assert M.round() is None             # ... and across a solve with the switch flipped in between
    mirror.set_option(framelib.OPT_COPY_BACK, 0); M.copy_back = False
    M.search(1)
    mirror.set_option(framelib.OPT_COPY_BACK, 1); M.copy_back = True
    assert M.round() is None
    M.close()


def test_nn_method_switched_at_unchanged_poses(mirror, orc, pb):
    M = mc.Model(mirror, orc, pb)
    for method in (L.NN_AUTO, L.NN_GRID, L.NN_TILE, L.NN_BRUTE, L.NN_AUTO):
        mirror.set_option(framelib.OPT_NN_METHOD, method); M.nn_method = method
        for i in (1, 2, 3):
            M.search(i)
    assert M.solve() is None
    M.close()


def test_copy_threads_one_and_eight_above_the_pooled_threshold(mirror, orc):
    """make_problem(3, 36000): frames 1 and 2 hold 71872 and 70920 triples at the initial poses (the oracle's filter on the real nanoflann's
    answers, counted when this test was written) -- more than the 65536 triples = 1 MiB below which parallel_copy stays on the calling
    thread.  copy_threads 1 and 8 fill identical bytes, equal to Engine.map_correspondences."""
    big = synth.make_problem(3, 36000)
    filled = {}
    for threads in (1, 8):
        M = mc.Model(mirror, orc, big, reference="engine")
        mirror.set_option(framelib.OPT_COPY_THREADS, threads)
        for i in range(3):
            M.search(i)
        per_frame = [sum(len(t) for _, _, t in M.expect[s]) for s in M.slots]
        print("triples per frame:", per_frame)
        assert max(per_frame) > 65536, per_frame     # from the reference's counts: below this the pooled path does not run
        filled[threads] = [[lst.tobytes() for _, _, lst in mirror.get_edges(s)] for s in M.slots]
        M.close()
    assert filled[1] == filled[8]


# ---------------------------------------------------------------- C: a bound frame changes
def bound(mirror, orc, pb):
    M = mc.Model(mirror, orc, pb)
    assert M.round() is None
    return M


def test_bound_pts_replaced(mirror, orc, pb, other):
    M = bound(mirror, orc, pb)
    M.store(M.slots[2], other["pts"][2], other["nor"][2])                   # (a): another size
    assert M.round() is None
    M.store(M.slots[2], other["pts"][1], other["nor"][1])                   # (b): the same size, another buffer
    assert M.round() is None
    M.store(M.slots[1], pb["pts"][1][::-1].copy(), pb["nor"][1][::-1].copy())   # (b) on a frame that kept its size since the first upload
    assert M.round() is None
    M.close()


def test_bound_nor_replaced_dropped_reattached(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    s = M.slots[2]
    flipped = np.ascontiguousarray(-pb["nor"][2])
    M.store_nor(s, flipped)
    assert M.round() is None
    M.store_nor(s, None)                  # dropped: a point-to-plane solve now lacks the normals of a destination
    for i in range(4):
        M.search(i)
    err = M.solve()
    assert err is not None and "needs normals" in str(err)
    assert M.solve(plane=False) is None   # (the refused solve left the session usable)
    M.store_nor(s, pb["nor"][2])
    assert M.round() is None
    M.close()


def test_bound_recompute_normals(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    s = M.slots[3]
    mirror.recompute_normals(s)
    got = mirror.get_nor(s)
    assert mc.same_bytes(got, mc.reference_normals(pb["pts"][3]))
    M.nor[s] = got; M.drop_twin()         # (the version moved: the mirror uploads the new normals by itself)
    assert mirror.get_version(s) == 1
    assert M.round() is None
    M.close()


def test_bound_in_place_overwrite_then_invalidate(mirror, orc, pb, other):
    M = bound(mirror, orc, pb)
    s = M.slots[1]
    n = len(pb["pts"][1])
    M.store(s, np.vstack([other["pts"][1], other["pts"][2][:n - 1200]]), np.vstack([other["nor"][1], other["nor"][2][:n - 1200]]), framelib.IN_PLACE)
    mirror.invalidate()
    assert M.round() is None
    M.close()


def test_bound_fixed_toggled(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    mirror.set_fixed(M.slots[2], True)
    assert M.round() is None              # frame 2 keeps its lists and its pose
    mirror.set_fixed(M.slots[2], False)
    assert M.round() is None
    M.close()


def test_bound_neighbours_rebuilt_with_three(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    M.pose_graph(3)
    assert sum(len(M.expect[s]) for s in M.slots) == 12
    assert M.round() is None
    assert M.round() is None
    M.close()


def test_second_vector_over_the_same_frames(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    mirror.vec_set(1, M.slots)
    for v in (1, 0, 1):
        M.drop_twin()                     # (another vector object: the mirror uploads again)
        for i in range(4):
            M.search(i, v)
        assert M.solve(v=v) is None
    M.close()


def test_frame_appended_and_two_frames_swapped(mirror, orc, pb, other):
    M = bound(mirror, orc, pb)
    five = synth.make_problem(5, 1500)
    s = M.new_frame(five["pts"][4], five["nor"][4], five["init"][4])
    M.set_vector(M.slots + [s])
    M.pose_graph(2)
    assert M.round() is None
    a = list(M.slots)
    a[1], a[3] = a[3], a[1]
    M.set_vector(a)                       # neighbour indices are positions: the same numbers now name other frames
    assert M.round() is None
    M.pose_graph(2)
    assert M.round() is None
    M.close()


def test_overlap_neighbours_then_the_loop(mirror, orc, pb):
    M = mc.Model(mirror, orc, pb)
    comps = mirror.overlap_neighbours(0, 2, mc.THRESH, 512, 0.0)
    eng = mc.fresh_engine(*M.clouds())
    ov = eng.overlap(M.poses(), mc.THRESH, 512)
    eng.close()
    src, dst, want_comps = mvicp.graph_from_overlap(ov["samples"], ov["hits"], ov["sumq"], 2, 0.0, skip_fixed0=False, cap=16)
    assert comps == want_comps
    for i, s in enumerate(M.slots):
        got = mirror.get_edges(s)
        assert [g[0] for g in got] == [int(d) for a, d in zip(src, dst) if a == i]
        for nb, w, lst in got:
            assert w == np.float32(1) - np.float32(ov["hits"][i, nb] / ov["samples"][i]) and len(lst) == 0
    M.take_graph()
    assert M.round() is None
    assert M.round() is None
    M.close()


def test_fused_model_between_two_rounds(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    gp, gn = mirror.fused_model(0, 0.01)
    eng = mc.fresh_engine(*M.clouds())
    want = eng.voxel_grid(0.01, None, M.poses())
    eng.close()
    assert len(gp) > 100 and mc.same_bytes(gp, want["xyz"]) and mc.same_bytes(gn, want["nrm"])
    assert M.round() is None
    M.close()


def test_bound_frame_recreated_in_the_same_storage(mirror, orc, pb, other):
    """Issue item 3 on a bound frame: the Frame of slot 2 is destroyed and another one constructed at its address (version 0 again)."""
    M = bound(mirror, orc, pb)
    s = M.slots[2]
    pose, addr = mirror.get_pose(s), mirror.slot_address(s)
    mirror.slot_destroy(s); mirror.slot_recreate(s)
    assert mirror.slot_address(s) == addr and mirror.get_version(s) == 0
    M.store(s, other["pts"][2], other["nor"][2])
    mirror.set_pose(s, pose)
    mirror.set_neighbours(s, [nb for nb, _, _ in M.expect[s]], [w for _, w, _ in M.expect[s]])
    M.expect[s] = [[nb, w, mc.EMPTY] for nb, w, _ in M.expect[s]]
    assert M.round() is None
    M.close()


# ---------------------------------------------------------------- D: unbound frames and the side context
def unbound(mirror, cloud, nor=None):
    s = mirror.slot_create()
    mirror.set_pts(s, cloud)
    mirror.set_nor(s, nor)
    return s


def test_side_context_follows_the_frame_and_its_cloud(mirror, orc, refnn, pb, other):
    x, y = unbound(mirror, pb["pts"][1]), unbound(mirror, pb["pts"][2])
    mc.check_nn(mirror, orc, refnn, x, pb["pts"][1])
    mc.check_nn(mirror, orc, refnn, y, pb["pts"][2])
    mc.check_nn(mirror, orc, refnn, x, pb["pts"][1])
    small = np.ascontiguousarray(other["pts"][0][:700])
    mirror.set_pts(x, small)                                            # (a): a smaller cloud -- every index below pts.size()
    mc.check_nn(mirror, orc, refnn, x, small)
    swapped = np.ascontiguousarray(other["pts"][3][:700])
    mirror.set_pts(x, swapped)                                          # (b)
    mc.check_nn(mirror, orc, refnn, x, swapped)
    addr = mirror.slot_address(x)
    mirror.slot_destroy(x); mirror.slot_recreate(x)                     # item 3: another Frame at the same address, version 0 again
    assert mirror.slot_address(x) == addr
    mirror.set_pts(x, other["pts"][1])
    mc.check_nn(mirror, orc, refnn, x, other["pts"][1])
    mirror.set_pts(x, other["pts"][2], framelib.IN_PLACE)               # (c) + invalidate()
    mirror.invalidate()
    mc.check_nn(mirror, orc, refnn, x, other["pts"][2])


def test_stages_on_an_unbound_frame(mirror, pb):
    pts, nor = pb["pts"][1], pb["nor"][1]
    x = unbound(mirror, pts, nor)
    mc.check_stages(mirror, x, pts, nor)
    mirror.recompute_normals(x)
    pca = mirror.get_nor(x)
    assert mc.same_bytes(pca, mc.reference_normals(pts)) and not mc.same_bytes(pca, nor)
    mc.check_stages(mirror, x, pts, pca)
    flipped = np.ascontiguousarray(-nor)
    mirror.set_nor(x, flipped)                                          # nor replaced
    mc.check_stages(mirror, x, pts, flipped)
    mirror.set_nor(x, None)
    mc.check_stages(mirror, x, pts, None)


def test_stages_and_queries_on_bound_frames(mirror, orc, refnn, pb, other):
    M = bound(mirror, orc, pb)
    s = M.slots[2]
    mc.check_nn(mirror, orc, refnn, s, pb["pts"][2])
    mc.check_stages(mirror, s, pb["pts"][2], pb["nor"][2])
    mirror.recompute_normals(s)
    pca = mirror.get_nor(s)
    mc.check_stages(mirror, s, pb["pts"][2], pca)                       # (the session still holds the old normals)
    flipped = np.ascontiguousarray(-pb["nor"][2])
    M.store_nor(s, flipped)
    mc.check_stages(mirror, s, pb["pts"][2], flipped)
    M.store(s, other["pts"][0], other["nor"][0])                        # its cloud replaced while the session holds the old one
    mc.check_nn(mirror, orc, refnn, s, other["pts"][0])
    mc.check_stages(mirror, s, other["pts"][0], other["nor"][0])
    mc.check_nn(mirror, orc, refnn, M.slots[1], pb["pts"][1])           # another bound frame, untouched
    assert M.round() is None
    mc.check_nn(mirror, orc, refnn, s, other["pts"][0])
    M.close()


def test_queries_after_the_bound_vector_is_destroyed(mirror, orc, refnn, pb):
    M = bound(mirror, orc, pb)
    slots = list(M.slots)
    M.drop_twin()
    mirror.vec_destroy(0)
    for i in (3, 1):
        mc.check_nn(mirror, orc, refnn, slots[i], pb["pts"][i])
        mc.check_stages(mirror, slots[i], pb["pts"][i], pb["nor"][i])
    mirror.slot_destroy(slots[2])                                       # ... and one of the frames it held ends too
    mc.check_nn(mirror, orc, refnn, slots[1], pb["pts"][1])
    mc.check_stages(mirror, slots[3], pb["pts"][3], pb["nor"][3])


# ---------------------------------------------------------------- E: getNeighbours
def check_knn(mirror, slot, cloud, k):
    _, want = mc.reference_normals(cloud, k, want_knn=True)
    got = mirror.get_neighbour_indices(slot, k, len(cloud))
    assert mc.same_bytes(got, want), k
    for q in (0, len(cloud) // 2, len(cloud) - 1):
        assert mc.same_bytes(mirror.get_neighbours(slot, q, k), cloud[want[q]])
        assert want[q][0] == q


def test_get_neighbours_tables(mirror, pb, other):
    x = unbound(mirror, pb["pts"][1])
    for k in (3, 10, 16, 10):
        check_knn(mirror, x, pb["pts"][1], k)
    mirror.set_pts(x, other["pts"][1])                                  # (a)
    check_knn(mirror, x, other["pts"][1], 10)
    mirror.set_pts(x, other["pts"][2])                                  # (b)
    check_knn(mirror, x, other["pts"][2], 10)
    mirror.set_pts(x, other["pts"][3], framelib.IN_PLACE)               # (c): Session::invalidate() drops the table
    mirror.invalidate()
    check_knn(mirror, x, other["pts"][3], 10)


def test_get_neighbours_refusals(mirror, pb):
    x = unbound(mirror, pb["pts"][1])
    few = unbound(mirror, pb["pts"][2][:12])
    for slot, k in ((x, 2), (x, 17), (few, 13)):
        with pytest.raises(framelib.MirrorError, match=r"getNeighbours supports 3 <= num_results <= 16 \(and <= the cloud's size\)"):
            mirror.get_neighbour_indices(slot, k, 12 if slot == few else 1500)
    bad = pb["pts"][3].copy()
    bad[77, 1] = np.nan
    y = unbound(mirror, bad)
    with pytest.raises(framelib.MirrorError, match="non-finite coordinate in cloud"):   # the library's message, not an empty or a later one
        mirror.get_neighbour_indices(y, 10, len(bad))
    with pytest.raises(framelib.MirrorError, match="non-finite coordinate in cloud"):
        mirror.recompute_normals(y)
    check_knn(mirror, x, pb["pts"][1], 10)


# ---------------------------------------------------------------- F: after a throw
def test_refused_upload_then_the_old_vector_moved_back(mirror, orc, pb):
    """Issue item 4: the upload of a NaN cloud on frame 2 is refused after mvicp_set_num_frames has emptied the context."""
    M = bound(mirror, orc, pb)
    s = M.slots[2]
    bad = pb["pts"][2].copy()
    bad[5, 0] = np.inf
    mirror.stash_set(bad)
    mirror.stash_swap_pts(s)               # the frame holds the bad cloud, the harness keeps the old VECTOR (buffer and all)
    with pytest.raises(framelib.MirrorError, match="non-finite coordinate in cloud"):
        mirror.closest_to_neighbours(0, 1, mc.THRESH)
    with pytest.raises(framelib.MirrorError, match="non-finite coordinate in cloud"):
        mirror.ceres(0)
    mirror.stash_swap_pts(s)               # the old vector moved back: the same buffer address and size the session last uploaded
    assert mc.same_bytes(mirror.get_pts(s), pb["pts"][2])
    M.drop_twin()
    assert M.round() is None
    M.close()


def test_refused_symmetric_solve(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    M.store_nor(M.slots[3], None)
    for i in range(4):
        M.search(i)
    with pytest.raises(framelib.MirrorError, match="symmetric needs normals on frame 3"):
        mirror.optimize(0, L.PARAM_SOPHUS_SE3, L.METRIC_SYMMETRIC)
    assert M.solve(plane=False) is None
    assert M.round(plane=False) is None
    M.close()


def test_refused_feature_init_with_voxel_copies(mirror, orc, pb):
    M = bound(mirror, orc, pb)
    P0 = M.poses()
    with pytest.raises(framelib.MirrorError, match="radius must be finite and > 0"):
        mirror.init_from_features(0, voxel=0.01, radius=0.0, tau=0.015)
    assert mc.same_bytes(M.poses(), P0)
    M.drop_twin()                          # (the session held the voxel copies: the next call uploads the frames)
    assert M.round() is None
    M.close()


def test_query_on_an_empty_frame(mirror, orc, refnn, pb):
    x = unbound(mirror, pb["pts"][1])
    mc.check_nn(mirror, orc, refnn, x, pb["pts"][1])
    empty = mirror.slot_create()
    with pytest.raises(framelib.MirrorError, match="getClosestPoint on an empty cloud"):
        mirror.get_closest_point(empty, [0.0, 0.0, 0.4])
    with pytest.raises(framelib.MirrorError, match="getClosestPoint on an empty cloud"):
        mirror.get_closest_points(empty, pb["pts"][1][:4])
    mc.check_nn(mirror, orc, refnn, x, pb["pts"][1])
    mirror.set_pts(empty, pb["pts"][2])
    mc.check_nn(mirror, orc, refnn, empty, pb["pts"][2])
