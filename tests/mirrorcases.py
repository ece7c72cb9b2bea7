"""What tests/test_gpu_frame_mirror.py shares: a Python-side model of the frames the harness holds (tests/framelib.py), the references
the mirror's answers are compared with, and the twin engine that is driven with the same searches and solves.

The references are independent of the mirror (host/frame.cpp): correspondence lists and weights come from the CPU oracle
(orc.correspond_edge) on the clouds the test stored and the poses the frames hold at that moment; poses after a solve from a twin
mvicp.Engine that is created whenever the clouds or the graph change -- that is, whenever the mirror has to upload again -- and is then
driven with the same searches and solves."""
import numpy as np

import framelib
import mvicp
from mvicp import lib as L
from mvicp import synth

THRESH = 0.05
EMPTY = np.zeros(0, dtype=framelib.CORR_DTYPE)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def triples(first, second, dist):
    t = np.zeros(len(first), dtype=framelib.CORR_DTYPE)
    t["first"], t["second"], t["dist"] = first, second, dist
    return t


def fresh_engine(pts_list, nor_list):
    eng = mvicp.Engine(0)
    eng.set_frames(pts_list, nor_list)
    return eng


class Model:
    """The frames of vector 0 (and what each should hold), by slot.  reference = "oracle": lists from orc.correspond_edge;
    "engine": lists from the twin's Engine.map_correspondences (the large case, where the oracle's brute force would take too long)."""

    def __init__(self, mirror, orc, pb=None, knn=2, reference="oracle", thresh=THRESH):
        self.m, self.orc, self.reference, self.thresh = mirror, orc, reference, thresh
        mirror.reset_all()
        self.slots = []                 # vector 0, in order
        self.pts, self.nor = {}, {}     # slot -> the cloud the test stored (nor: None when the frame has none)
        self.expect = {}                # slot -> [[neighbour, weight, triples], ...]: what the frame's edges should hold now
        self.copy_back, self.nn_method = True, L.NN_AUTO
        self.twin, self.twin_key, self.twin_lists = None, None, None
        if pb is not None:
            for i in range(len(pb["pts"])):
                self.slots.append(self.new_frame(pb["pts"][i], pb["nor"][i], pb["init"][i], i == 0))
            self.m.vec_set(0, self.slots)
            self.pose_graph(knn)

    def close(self):
        self.drop_twin()
        self.m.reset_all()

    # ---- frames
    def new_frame(self, pts, nor, pose, fixed=False):
        s = self.m.slot_create()
        self.store(s, pts, nor)
        self.m.set_pose(s, pose)
        self.m.set_fixed(s, fixed)
        self.expect[s] = []
        return s

    def store(self, s, pts, nor, mode=framelib.FRESH):
        """the cloud of slot s <- pts / nor (nor None: dropped).  The mirror has to notice (FRESH) or be told (IN_PLACE)."""
        self.m.set_pts(s, pts, mode)
        self.pts[s] = np.ascontiguousarray(pts, dtype=np.float64).copy()
        self.store_nor(s, nor, mode)

    def store_nor(self, s, nor, mode=framelib.FRESH):
        self.m.set_nor(s, nor, mode)
        self.nor[s] = None if nor is None else np.ascontiguousarray(nor, dtype=np.float64).copy()
        self.drop_twin()

    def set_vector(self, slots, v=0):
        self.m.vec_set(v, slots)
        if v == 0:
            self.slots = list(slots)
        self.drop_twin()

    def poses(self):
        return np.array([self.m.get_pose(s) for s in self.slots])

    def fixed(self):
        return np.array([self.m.get_fixed(s) for s in self.slots], dtype=np.uint8)

    def graph(self):
        src, dst = [], []
        for i, s in enumerate(self.slots):
            for nb, _, _ in self.expect[s]:
                src.append(i); dst.append(nb)
        return np.array(src, dtype=np.int32), np.array(dst, dtype=np.int32)

    def pose_graph(self, knn):
        """computePoseNeighboursKnn for every frame, checked against synth.pose_graph_knn (frame.cpp:67-89)."""
        for i in range(len(self.slots)):
            self.m.pose_knn(0, i, knn)
        P = self.poses()
        src, dst = synth.pose_graph_knn(P, knn, skip_fixed0=False)
        for i, s in enumerate(self.slots):
            want = [int(d) for a, d in zip(src, dst) if a == i]
            got = self.m.get_edges(s)
            assert [g[0] for g in got] == want, (i, got, want)
            for nb, w, lst in got:
                assert w == np.float32(np.linalg.norm(P[i][:3, 3] - P[nb][:3, 3])) and len(lst) == 0
            self.expect[s] = [[nb, w, EMPTY] for nb, w, _ in got]
        self.drop_twin()

    def take_graph(self):
        """the model's expectation <- the neighbours the frames hold now (after a call that rebuilt them; checked by the caller)"""
        for s in self.slots:
            self.expect[s] = [[nb, w, lst] for nb, w, lst in self.m.get_edges(s)]
        self.drop_twin()

    # ---- the twin
    def drop_twin(self):
        if self.twin is not None:
            self.twin.close()
        self.twin, self.twin_key, self.twin_lists = None, None, None

    def clouds(self):
        pts = [self.pts[s] for s in self.slots]
        nor = [self.nor[s] if self.nor[s] is not None and len(self.nor[s]) == len(self.pts[s]) else None for s in self.slots]
        return pts, nor

    def ensure_twin(self):
        if self.twin is None:
            self.twin = fresh_engine(*self.clouds())
            self.twin.set_graph(*self.graph())
        return self.twin

    def twin_search(self):
        P, fx = self.poses(), self.fixed()
        key = (P.tobytes(), fx.tobytes(), self.thresh, self.nn_method)
        twin = self.ensure_twin()
        if key != self.twin_key:
            counts, weights = twin.correspond(P, fx, self.thresh, self.nn_method)
            self.twin_key = key
            self.twin_lists = (twin.map_correspondences(), weights) if self.reference == "engine" else None

    def reference_edge(self, i, j, e):
        """-> (triples, weight) of edge j of the frame at position i (edge e of the graph) at the current poses"""
        if self.reference == "engine":
            (t, off), weights = self.twin_lists
            return t[off[e]:off[e + 1]].copy(), np.float32(weights[e])
        s = self.slots[i]
        d = self.slots[self.expect[s][j][0]]
        f, sec, dist, w, _, _ = self.orc.correspond_edge(self.pts[s], self.m.get_pose(s), self.pts[d], self.m.get_pose(d), self.thresh)
        return triples(f, sec, dist), np.float32(w)

    # ---- the reference's two calls
    def search(self, i, v=0):
        """computeClosestPointsToNeighbours of the frame at position i -> (edges copied, edges skipped).  Afterwards EVERY frame holds what the
        model expects: the called one the reference's lists and weights, the others what they had."""
        s = self.slots[i]
        fixed = self.m.get_fixed(s)
        if not fixed:
            self.twin_search()
        c0, k0 = self.m.counters()
        self.m.closest_to_neighbours(v, i, self.thresh)
        c1, k1 = self.m.counters()
        n_edges = len(self.expect[s])
        if fixed:
            assert (c1 - c0, k1 - k0) == (0, 0)   # frame.cpp:93: a fixed frame is not searched
        else:
            assert (c1 - c0) + (k1 - k0) == n_edges, (c1 - c0, k1 - k0, n_edges)
            e0 = sum(len(self.expect[t]) for t in self.slots[:i])
            for j in range(n_edges):
                t, w = self.reference_edge(i, j, e0 + j)
                self.expect[s][j] = [self.expect[s][j][0], w, t if self.copy_back else EMPTY]
        self.check_all()
        return c1 - c0, k1 - k0

    def check_all(self):
        for i, s in enumerate(self.slots):
            got = self.m.get_edges(s)
            assert len(got) == len(self.expect[s]), (i, len(got), len(self.expect[s]))
            for j, ((nb, w, lst), (enb, ew, elst)) in enumerate(zip(got, self.expect[s])):
                assert nb == enb, (i, j, nb, enb)
                assert np.float32(w).tobytes() == np.float32(ew).tobytes(), ("weight", i, j, w, ew)
                assert len(lst) == len(elst), ("count", i, j, len(lst), len(elst))
                assert lst.tobytes() == elst.tobytes(), ("list", i, j)

    def solve(self, which=framelib.CERES_SOPHUS, plane=True, robust=True, v=0):
        """ICP_Ceres::ceresOptimizer* on vector v against the twin's solve from the same poses -> the mirror's exception or None.
        Both refuse or neither; the poses afterwards are the twin's, byte for byte."""
        P0, fx = self.poses(), self.fixed()
        want, err_twin, err = None, None, None
        try:
            want, _ = self.ensure_twin().optimize(P0, fx, which, plane, robust, 50)
        except mvicp.MvicpError as ex:
            err_twin = ex
        try:
            self.m.ceres(v, which, plane, robust)
        except framelib.MirrorError as ex:
            err = ex
        assert (err is None) == (err_twin is None), (err, err_twin)
        if err is not None:
            assert str(err_twin).split(": ", 1)[1] in str(err), (err, err_twin)   # the library's message reaches the caller
            assert same_bytes(self.poses(), P0)
            return err
        assert_poses(self.poses(), want)
        return None

    def round(self, order=None, **kw):
        """one search per frame, then one solve (main_multiview.cpp:119-131)"""
        for i in (range(len(self.slots)) if order is None else order):
            self.search(i)
        return self.solve(**kw)


def assert_poses(got, want):
    print("poses: max |mirror - twin| = %.3e" % float(np.abs(np.asarray(got) - np.asarray(want)).max()))
    assert same_bytes(got, want)


def queries_near(cloud, n, seed):
    """n query points: points of the cloud pushed off by up to a few millimetres (every coordinate of the cloud's scale)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pick = rng.integers(0, len(cloud), n)
    return np.ascontiguousarray(cloud[pick] + rng.normal(0, 3e-3, (n, 3)))


def check_nn(mirror, orc, refnn, slot, cloud, seed=7, n=160):
    """getClosestPoints and getClosestPoint of the frame in `slot` against the oracle (and the real nanoflann) on `cloud`"""
    Q = queries_near(cloud, n, seed)
    idx, d2 = mirror.get_closest_points(slot, Q)
    assert idx.max() < len(cloud) and idx.min() >= 0, (idx.max(), len(cloud))
    ri, rd = orc.nn_brute(cloud, Q)
    assert np.array_equal(idx, ri) and same_bytes(d2, rd)
    if refnn is not None:
        ni, nd = refnn.query(cloud, Q)
        assert np.array_equal(idx, ni) and same_bytes(d2, np.asarray(nd, dtype=np.float64))
    for k in range(3):
        i1, d1 = mirror.get_closest_point(slot, Q[k])
        assert i1 == ri[k] and np.float64(d1).tobytes() == np.float64(rd[k]).tobytes()


VOXEL = 0.01
OUTLIER = (8, 1.0, 0.0)
ISS = (0.04, 0.02, 0.9, 0.9, 3)


def check_stages(mirror, slot, pts, nor):
    """voxelDownsample, removeOutliers and issKeypoints of the frame in `slot` against the same stages of a fresh engine that holds
    `pts` / `nor` (None: no normals)"""
    eng = fresh_engine([pts], [nor])
    try:
        v = eng.voxel_grid(VOXEL, frames=[0])
        o = eng.outlier_filter(0, *OUTLIER)
        k = eng.iss_keypoints(0, *ISS)
    finally:
        eng.close()
    gp, gn = mirror.voxel_downsample(slot, VOXEL)
    assert same_bytes(gp, v["xyz"]) and (gn is None) == (v["nrm"] is None) and (gn is None or same_bytes(gn, v["nrm"])), "voxelDownsample"
    gp, gn = mirror.remove_outliers(slot, *OUTLIER)
    assert same_bytes(gp, o["xyz"]) and (gn is None) == (o["nrm"] is None) and (gn is None or same_bytes(gn, o["nrm"])), "removeOutliers"
    assert 0 < len(o["xyz"]) < len(pts)
    assert same_bytes(mirror.iss_keypoints(slot, *ISS), k["idx"]), "issKeypoints"


def reference_normals(pts, k=10, want_knn=False):
    eng = fresh_engine([pts], None)
    try:
        return eng.recompute_normals(0, k, want_knn)
    finally:
        eng.close()
