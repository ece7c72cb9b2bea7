"""mvicp_cluster / mvicp_cluster_fetch / mvicp_cluster_select / mvicp_cluster_fetch_kept on the MI355X: label, core, size and every number of
the stats equal the numpy statement of the contract (tests/clusterref.py) byte for byte, and after a selection so do xyz, nrm, idx and label.
What a case must contain (core, border and noise, exact ties, a chain of thousands of links, every way out of the traversal) is asserted on
the reference alone, so no case can pass by calling everything noise or one cluster."""
import ctypes as C
import functools

import numpy as np
import pytest

import clusterref as cr
import mvicp
import outlierref
import traverseref
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3
RULES = ((0, 0), (100, 0), (0, 1), (2, 3))   # (min_size, max_clusters) of the selections every case is put through


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def check(eng, p, nrm, radius, min_pts, what, rules=RULES, device=False, frame=0):
    """cluster + every selection of `rules` on the engine's frame against the reference -> the reference result."""
    want = reference(p, radius, min_pts, nrm is not None)
    got = _host(eng.cluster(frame, radius, min_pts, device=device))
    print(what, "radius", radius, "min_pts", min_pts, got["stats"])
    assert cr.same(got, want), (what, min_pts, got["stats"], want["stats"], int((got["label"] != want["label"]).sum()), int((got["core"] != want["core"]).sum()))
    for rule in rules:
        sel = _host(eng.cluster_select(*rule, device=device))
        ws = cr.select(p, nrm, want, *rule)
        assert cr.same_kept(sel, ws), (what, min_pts, rule, sel["kept"], ws["kept"])
    return want


_REF = {}


def reference(p, radius, min_pts, normals):
    """The reference result of a cloud, computed once per (bytes, radius, min_pts) and shared; nobody writes into it."""
    key = (p.tobytes(), float(radius), int(min_pts), bool(normals))
    if key not in _REF:
        r = cr.cluster(p, np.zeros((len(p), 3)) if normals else None, radius, min_pts)
        for a in (r["label"], r["core"], r["size"]):
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


@functools.lru_cache(maxsize=None)
def blobs():
    return cr.blobs_cloud()


@pytest.mark.parametrize("min_pts", [1, 5, 17, 40])
def test_blobs(eng, min_pts):
    """Three blobs in uniform clutter; min_pts = 40 is beyond the 33-entry lists of the outlier kernel: the count has no list."""
    p, nr = blobs()
    want = reference(p, cr.BLOBS_RADIUS, min_pts, True)
    s = want["stats"]
    if min_pts == 1:
        assert s["clusters"] > 100 and s["noise"] == 0 and s["border"] == 0
    else:
        assert s["clusters"] == 3 and s["core"] > 0 and s["border"] > 0 and s["noise"] > 0
    eng.set_frames([p], [nr])
    check(eng, p, nr, cr.BLOBS_RADIUS, min_pts, "blobs")


def test_sheet_and_clump(eng):
    p, nr = cr.sheet_clump_cloud()
    want = reference(p, cr.SHEET_RADIUS, cr.SHEET_MIN_PTS, True)
    assert want["size"].tolist() == [3000, 40] and want["stats"]["noise"] == 0
    assert (want["label"][:3000] == 0).all() and (want["label"][3000:] == 1).all()          # the clump is one whole cluster of its own
    # what the two outlier rules make of it (the reason this stage exists): both keep every clump point
    assert (outlierref.outlier_filter(p, None, 8, 2.0, 0.0)["idx"] >= 3000).sum() == 40
    assert (outlierref.outlier_filter(p, None, 8, -1.0, 0.03)["idx"] >= 3000).sum() == 40
    eng.set_frames([p], [nr])
    check(eng, p, nr, cr.SHEET_RADIUS, cr.SHEET_MIN_PTS, "sheet + clump")
    for rule in ((100, 0), (0, 1)):
        sel = eng.cluster_select(*rule)
        assert sel["kept"] == 3000 and sel["idx"].tolist() == list(range(3000)) and sel["xyz"].tobytes() == p[:3000].tobytes()
        assert sel["nrm"].tobytes() == nr[:3000].tobytes() and (sel["label"] == 0).all()


def _tied_border_points(p, radius, res):
    """Border points whose first two core neighbours in the order (d2, index) are exactly as far."""
    A, out = cr.adjacency(p, radius), []
    for i in np.flatnonzero((res["core"] == 0) & (res["label"] >= 0)):
        js = np.flatnonzero(A[i] & (res["core"] == 1))
        d = ((p[i] - p[js]) ** 2)
        d = (d[:, 0] + d[:, 1]) + d[:, 2]
        if (d == d.min()).sum() > 1:
            out.append(int(i))
    return out


def test_dyadic_lattice(eng):
    """8 x 8 x 2 points at pitch 2^-8: every distance is exact.  radius = pitch: strictness makes n singletons.  The next double: one
    cluster.  At that radius a point has itself, up to four neighbours in its layer and one in the other: 6 in the interior, 5 on an edge,
    4 in a corner.  So min_pts = 5 leaves the 8 corners as border points, each exactly one pitch from two core points of its layer (the tie
    the lower index decides), and no noise; min_pts = 6 makes the interior the core, the edges its border and the corners noise; min_pts =
    7 has no core point at all (the case as the issue words it -- an interior-only core with tied border points and no noise at 7 -- does
    not exist on this lattice: 5 and 6 hold its parts, and 7 is run as well)."""
    p = cr.dyadic_lattice()
    R = float(np.nextafter(cr.LATTICE_PITCH, 1.0))
    assert reference(p, cr.LATTICE_PITCH, 1, False)["stats"]["clusters"] == len(p)
    assert reference(p, R, 1, False)["stats"]["clusters"] == 1
    w5, w6, w7 = (reference(p, R, m, False) for m in (5, 6, 7))
    assert (w5["stats"]["core"], w5["stats"]["border"], w5["stats"]["noise"]) == (120, 8, 0) and len(_tied_border_points(p, R, w5)) == 8
    xy = np.round(p / cr.LATTICE_PITCH).astype(int)[:, :2]
    interior = ((xy >= 1) & (xy <= 6)).all(1)
    assert ((w6["core"] == 1) == interior).all() and w6["stats"]["border"] == 48 and w6["stats"]["noise"] == 8
    assert w7["stats"]["clusters"] == 0 and w7["stats"]["noise"] == len(p)
    eng.set_frames([p], None)
    check(eng, p, None, cr.LATTICE_PITCH, 1, "lattice, radius = pitch")
    for m in (1, 5, 6, 7):
        check(eng, p, None, R, m, "lattice")
    # the same ties with the index order turned round: the OTHER neighbour wins
    q = np.ascontiguousarray(p[::-1])
    eng.set_frames([q], None)
    assert len(_tied_border_points(q, R, reference(q, R, 5, False))) == 8
    check(eng, q, None, R, 5, "lattice reversed")


def test_bridge(eng):
    p, mid = cr.bridge_cloud()
    want = reference(p, cr.BRIDGE_RADIUS, cr.BRIDGE_MIN_PTS, False)
    assert want["stats"]["clusters"] == 2 and want["stats"]["noise"] == 0 and not want["core"][mid]
    line = [int(np.flatnonzero((p == np.array([x, 1, 1]) * cr.BRIDGE_PITCH).all(1))[0]) for x in (4, 5, 6)]
    assert line[1] == mid and not want["core"][line].any()                                   # the line's neighbourhoods stay below min_pts
    near = np.flatnonzero(cr.adjacency(p, cr.BRIDGE_RADIUS)[mid] & (want["core"] == 1))
    d = cr.dist2_slab(p, 0)[mid][near]
    first = near[d == d.min()]
    assert len(first) == 2 and want["label"][first[0]] != want["label"][first[1]] and want["label"][mid] == want["label"][first.min()]
    eng.set_frames([p], None)
    check(eng, p, None, cr.BRIDGE_RADIUS, cr.BRIDGE_MIN_PTS, "bridge")


@pytest.mark.parametrize("order", ["index", "reversed", "shuffled"])
def test_helix(eng, order):
    """A chain of 4 095 links: in index order every hook lands on the root of the chain so far, reversed every point is its own root
    until the last, shuffled the trees meet in the middle."""
    p = cr.helix_cloud(4096, order)
    radius = 1.5 * cr.HELIX_STEP
    w2, w3 = reference(p, radius, 2, False), reference(p, radius, 3, False)
    assert w2["stats"]["clusters"] == 1 and w2["stats"]["core"] == 4096
    assert w3["stats"]["clusters"] == 1 and w3["stats"]["core"] == 4094 and w3["stats"]["border"] == 2
    eng.set_frames([p], None)
    check(eng, p, None, radius, 2, "helix " + order, rules=((0, 0),))
    check(eng, p, None, radius, 3, "helix " + order, rules=((0, 1),))


def test_degenerate_and_off_origin_inputs(eng):
    same = np.tile([[0.25, -0.5, 1.0]], (200, 1))
    eng.set_frames([same], None)
    for m, clusters in ((1, 1), (200, 1), (201, 0)):
        want = check(eng, same, None, 0.01, m, "identical")
        assert want["stats"]["clusters"] == clusters and want["stats"]["noise"] == (0 if clusters else 200)
    line = cr.line_cloud()
    eng.set_frames([line], None)
    dims = eng.get_structure(0, "scalars")[:3]
    assert sorted(dims.tolist())[:2] == [2.0, 2.0], dims
    for m in (1, 3, 5):
        want = check(eng, line, None, 0.012, m, "line")
        assert want["stats"]["clusters"] > 1
    assert reference(line, 0.012, 5, False)["stats"]["noise"] > 0 and reference(line, 0.012, 5, False)["stats"]["border"] > 0
    p, nr = blobs()
    q = np.ascontiguousarray(p * 1e-3 + 1e3)
    eng.set_frames([q], [nr])
    for m in (1, 5, 17):
        want = check(eng, q, nr, cr.BLOBS_RADIUS * 1e-3, m, "blobs at scale 1e-3, offset 1e3", rules=((0, 0), (20, 2)))
        assert want["stats"]["clusters"] >= 3 and (m == 1 or want["stats"]["border"] > 0)


@pytest.mark.parametrize("kind", ["far", "corner"])
def test_every_way_out_of_the_traversal(eng, kind):
    """The radius passes stop once the block's faces lie a radius away; the radii are chosen from the grid the library built so that the
    points of "far" stop at the first block, at a larger one and not at all before the block exceeds 2 n cells (the cloud is scanned),
    and those of "corner" see their block cover the grid.  The kernels walk no box tree, like the outlier kernel."""
    p = traverseref.patch_cloud(kind)
    eng.set_frames([p], None)
    sc = eng.get_structure(0, "scalars")
    h = float(sc[6])
    seen = set()
    for f in (0.8, 2.5, 5.2):
        radius = f * h
        ways, radii, _ = traverseref.exits(p, sc, len(p), radius, tree=False)
        seen |= {(w, min(int(r), 2)) for w, r in zip(ways, radii)}
        print(kind, "cell", h, "dims", sc[:3], "radius", radius, {w: ways.count(w) for w in set(ways)})
        for m in (1, 4, 12):
            check(eng, p, None, radius, m, "patch " + kind, rules=((0, 0), (3, 2)))
    if kind == "far":
        assert {("stop", 1), ("stop", 2)} <= seen and any(w == "cloud" for w, _ in seen), seen
    else:
        assert any(w == "grid" for w, _ in seen), seen


def test_lattice_with_a_far_cluster(eng):
    """outlierref.lattice_cloud: 288 lattice points (exact ties) and five points 3 m away, whose blocks grow through empty cells."""
    p, nr = outlierref.lattice_cloud()
    eng.set_frames([p], [nr])
    for radius, m in ((0.0076, 1), (0.0076, 8), (0.0076, 19), (0.02, 6), (0.02, 5)):
        want = check(eng, p, nr, radius, m, "lattice + far cluster")
        assert (want["label"][288:] < 0).all() or want["label"][288] != want["label"][0]      # the far five never join the lattice
    assert reference(p, 0.02, 5, True)["stats"]["clusters"] == 2 and reference(p, 0.02, 6, True)["stats"]["clusters"] == 1


def test_small_n(eng):
    two = np.array([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]])
    eng.set_frames([np.zeros((0, 3)), two[:1], two], None)
    got = eng.cluster(0, 0.1, 1)
    assert got["label"].shape == (0,) and got["core"].shape == (0,) and got["size"].shape == (0,)
    assert got["stats"] == {"n": 0, "clusters": 0, "core": 0, "border": 0, "noise": 0, "largest": 0, "largest_label": -1, "has_normals": 0}
    sel = eng.cluster_select(0, 0)
    assert sel["kept"] == 0 and sel["xyz"].shape == (0, 3) and sel["idx"].shape == (0,)
    got = eng.cluster(0, 0.1, 1, device=True)
    assert got["label"].shape == (0,) and eng.cluster_select(5, 1, device=True)["xyz"].shape == (0, 3)
    for m, clusters in ((1, 1), (2, 0)):
        assert check(eng, two[:1], None, 0.1, m, "one point", frame=1)["stats"]["clusters"] == clusters
    for radius, m, clusters in ((0.0101, 1, 1), (0.0101, 2, 1), (0.0101, 3, 0), (0.01, 1, 2), (0.0099, 2, 0)):   # within, exactly at (strict) and beyond the radius
        assert check(eng, two, None, radius, m, "two points", frame=2)["stats"]["clusters"] == clusters
    # one workgroup of the compaction with a lane to spare, exactly full, and one point in a second workgroup: a selection in between,
    # then one cluster of everything kept whole (min_size 0) and dropped whole (min_size n + 1)
    for n, kept in ((255, 238), (256, 232), (257, 235)):
        p, nr, _ = outlierref.sheet_cloud(n, 100 + n)
        eng.set_frames([p], [nr])
        assert cr.select(p, nr, reference(p, 0.08, 4, True), 5, 0)["kept"] == kept
        check(eng, p, nr, 0.08, 4, "sheet of %d" % n, rules=((5, 0),))
        whole = reference(p, 10.0, 1, True)
        assert whole["stats"]["clusters"] == 1 and cr.select(p, nr, whole, 0, 0)["kept"] == n and cr.select(p, nr, whole, n + 1, 0)["kept"] == 0
        check(eng, p, nr, 10.0, 1, "sheet of %d, one cluster" % n, rules=((0, 0), (n + 1, 0)), device=(n == 256))


def test_frames_and_memory(eng):
    p, nr = blobs()
    s, sn = cr.sheet_clump_cloud()
    eng.set_frames([s, p], [sn, None])
    want = check(eng, p, None, cr.BLOBS_RADIUS, 5, "frame 1 of two, no normals", frame=1)
    assert want["stats"]["has_normals"] == 0 and eng.cluster_select(0, 0)["nrm"] is None
    buf = np.zeros((len(p), 3))
    st = eng.lib.mvicp_cluster_fetch_kept(eng.h, len(p), None, buf.ctypes.data_as(C.c_void_p), None, None)
    assert st == ERR_STATE and b"normals" in eng.lib.mvicp_last_error()
    check(eng, s, sn, cr.SHEET_RADIUS, cr.SHEET_MIN_PTS, "frame 0 of two", frame=0)
    # host and device uploads agree; device destinations refill; a device selection goes straight into another engine
    eng.set_frames_device([_dev(p)], [_dev(nr)])
    check(eng, p, nr, cr.BLOBS_RADIUS, 17, "device upload")
    check(eng, p, nr, cr.BLOBS_RADIUS, 17, "device upload, device fetch", device=True)
    check(eng, p, nr, cr.BLOBS_RADIUS, 5, "device fetch again", device=True)
    eng.cluster(0, cr.BLOBS_RADIUS, 5)
    dev, host = eng.cluster_select(100, 0, device=True), eng.cluster_select(100, 0)
    assert all(isinstance(dev[k], torch.Tensor) and dev[k].is_cuda for k in ("xyz", "nrm", "idx", "label"))
    a, b = mvicp.Engine(0), mvicp.Engine(0)
    try:
        a.set_frames_device([dev["xyz"]], [dev["nrm"]])
        b.set_frames([host["xyz"]], [host["nrm"]])
        for name in ("spts", "snor", "sidx"):
            assert a.get_structure(0, name).tobytes() == b.get_structure(0, name).tobytes(), name
        again = cr.cluster(host["xyz"], host["nrm"], cr.BLOBS_RADIUS, 5)
        assert again["stats"]["clusters"] == 3 and again["stats"]["n"] == host["kept"] < len(p)   # the three blobs without the clutter
        assert cr.same(a.cluster(0, cr.BLOBS_RADIUS, 5), again) and cr.same(b.cluster(0, cr.BLOBS_RADIUS, 5), again)
    finally:
        a.close(); b.close()


def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_clusters):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_clusters:
                e.cluster(2, 0.02, 4)   # before the graph exists
                e.cluster_select(10, 0)
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_clusters:
                    e.cluster(r, 0.03, 6)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_clusters:
                    e.cluster(3 - r, 0.01 if r else 0.05, 1 if r == 1 else 12, device=(r == 2))
                    e.cluster_select(50, 2, device=(r == 2))
                triples, offsets = e.map_correspondences()
                blocks = e.linearize(poses, True, True)
                if with_clusters:
                    e.cluster_select(0, 1)
                poses, sm = e.optimize(poses, pb["fixed"])
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_errors_and_empty_frame(eng):
    p = np.ascontiguousarray(blobs()[0][:600])
    want = cr.cluster(p, None, 0.03, 4)
    assert want["stats"]["clusters"] == 3 and want["stats"]["noise"] > 0
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        clu, fetch, select, kept = lib.mvicp_cluster, lib.mvicp_cluster_fetch, lib.mvicp_cluster_select, lib.mvicp_cluster_fetch_kept
        assert fetch(h, 10, None, None, 10, None) == ERR_STATE and select(h, 0, 0) == ERR_STATE      # before any cluster call
        assert kept(h, 10, None, None, None, None) == ERR_STATE
        assert clu(h, 0, 0.1, 4, None) == ERR_ARG                                                     # frames not declared: out of range
        assert lib.mvicp_set_num_frames(h, 4) == 0
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.mvicp_set_frame(h, 0, dp(p), None, len(p)) == 0
        assert lib.mvicp_set_frame(h, 2, dp(p), None, 0) == 0
        assert clu(h, 1, 0.03, 4, None) == ERR_STATE and b"never uploaded" in lib.mvicp_last_error()
        assert clu(h, 4, 0.03, 4, None) == ERR_ARG and clu(h, -1, 0.03, 4, None) == ERR_ARG
        S = mvicp.lib.ClusterStats()
        assert clu(h, 0, 0.03, 4, C.byref(S)) == want["stats"]["clusters"] and S.as_dict() == want["stats"]
        lab, core, size = np.zeros(len(p), np.int32), np.zeros(len(p), np.uint8), np.zeros(S.clusters, np.int32)

        def result_is_still_there():
            assert fetch(h, len(p), vp(lab), vp(core), S.clusters, vp(size)) == 0
            assert lab.tobytes() == want["label"].tobytes() and core.tobytes() == want["core"].tobytes() and size.tobytes() == want["size"].tobytes()

        result_is_still_there()
        assert kept(h, len(p), None, None, None, None) == ERR_STATE and b"select" in lib.mvicp_last_error()   # a result, but no selection yet
        # refused calls keep the earlier result: every argument error that is decided before the context is touched
        for args in ((0, 0.03, 0), (0, 0.03, -3), (0, 0.03, (1 << 30) + 1), (0, float("nan"), 4), (0, float("inf"), 4), (0, 0.0, 4), (0, -0.5, 4),
                     (4, 0.03, 4), (-1, 0.03, 4)):
            assert clu(h, args[0], args[1], args[2], None) == ERR_ARG, args
            result_is_still_there()
        assert clu(h, 0, 0.03, 1 << 30, None) == 0                                         # the largest min_pts: no core point, no cluster
        assert clu(h, 0, 0.03, 4, None) == S.clusters
        assert select(h, -1, 0) == ERR_ARG and select(h, 0, -1) == ERR_ARG
        ws = cr.select(p, None, want, 175, 0)
        assert 0 < ws["kept"] < len(p) and select(h, 175, 0) == ws["kept"]
        xyz, idx, kl = np.zeros((len(p), 3)), np.zeros(len(p), np.int32), np.zeros(len(p), np.int32)
        assert kept(h, ws["kept"] - 1, vp(xyz), None, None, None) == ERR_ARG                 # cap < kept
        assert fetch(h, len(p) - 1, vp(lab), None, 0, None) == ERR_ARG and fetch(h, len(p), None, None, S.clusters - 1, vp(size)) == ERR_ARG
        assert kept(h, ws["kept"], vp(xyz), None, vp(idx), vp(kl)) == 0
        assert xyz[:ws["kept"]].tobytes() == ws["xyz"].tobytes() and idx[:ws["kept"]].tobytes() == ws["idx"].tobytes()
        assert kl[:ws["kept"]].tobytes() == ws["label"].tobytes()
        # a neighbour distance that can overflow: reported by the call, and no result is left behind
        huge = np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [1.5e154, 0.0, 0.0]])
        assert cr.can_overflow(huge) and lib.mvicp_set_frame(h, 3, dp(huge), None, len(huge)) == 0
        assert clu(h, 3, 0.03, 1, None) == ERR_ARG and b"overflow" in lib.mvicp_last_error()
        assert fetch(h, 10, None, None, 10, None) == ERR_STATE and select(h, 0, 0) == ERR_STATE
        assert lib.mvicp_set_frame(h, 3, dp(p), None, 8) == 0
        # an empty frame is no error; an upload to the clustered frame ends the result; so does mvicp_set_num_frames
        assert clu(h, 2, 0.03, 4, C.byref(S)) == 0 and S.n == 0 and S.largest_label == -1 and select(h, 0, 0) == 0
        assert kept(h, 0, None, None, None, None) == 0
        assert clu(h, 0, 0.03, 4, None) == want["stats"]["clusters"]
        assert lib.mvicp_set_frame(h, 1, dp(p), None, len(p)) == 0 and fetch(h, len(p), vp(lab), None, 0, None) == 0   # another slot: stays
        assert lib.mvicp_set_frame(h, 0, dp(p), None, len(p)) == 0
        assert fetch(h, len(p), vp(lab), None, 0, None) == ERR_STATE and select(h, 0, 0) == ERR_STATE
        assert clu(h, 0, 0.03, 4, None) == want["stats"]["clusters"] and lib.mvicp_set_num_frames(h, 1) == 0
        assert fetch(h, 1 << 20, None, None, 1 << 20, None) == ERR_STATE
    finally:
        fresh.close()
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        eng.cluster(0, float("nan"), 4)
