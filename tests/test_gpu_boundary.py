"""mvicp_boundary / mvicp_boundary_fetch / mvicp_boundary_select / mvicp_boundary_fetch_kept on the MI355X: the flags, the counts and both
selections equal the numpy statement of the contract (tests/boundref.py) byte for byte, with host and with device destinations.  What a
case must contain (flagged, unflagged and undecided points) is asserted on the reference alone in
tests/test_boundary_cpu.py::test_the_cases_hold_what_they_are_for and, in short, here, so no case can pass by flagging nothing."""
import ctypes as C

import numpy as np
import pytest

import boundref as br
import mvicp
from boundref import reference
from mvicp import synth

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def check(eng, p, stored, want, args, what, source=0, frame=0, devices=(False, True)):
    """boundary and both selections on the engine's frame against the reference `want`, with host and with device destinations; stored =
    the frame's stored normals (None: none), which the selections carry"""
    for device in devices:
        got = _host(eng.boundary(frame, *args, source=source, device=device))
        if not device:
            print(what, args, "flagged", got["boundary"], "of", len(p), "undecided or without a direction", int((got["valid"] == 0).sum()))
        assert br.same(got, want), (what, args, device, got["boundary"], want["boundary"], {k: int((got[k] != want[k]).sum()) for k, _ in br.KEYS})
        for boundary in (True, False):
            sel = _host(eng.boundary_select(boundary, device=device))
            ws = br.select(p, stored, want, boundary)
            assert br.same_kept(sel, ws), (what, args, boundary, device, sel["kept"], ws["kept"])


def run_case(eng, name, devices=(False, True)):
    p, N, runs = br.cases()[name]
    eng.set_frames([p], [N])
    for r, args in enumerate(runs):
        check(eng, p, N, reference(name, r), args, name, devices=devices)


def test_blob(eng):
    assert [reference("blob", r)["boundary"] for r in range(3)] == [2000, 783, 39]   # k = 3: two directions always leave a gap
    run_case(eng, "blob")


def test_e2e_dst(eng):
    assert [reference("e2e dst", r)["boundary"] for r in range(2)] == [130, 184]
    run_case(eng, "e2e dst")


def test_lattice_shuffled(eng):
    k5, k9 = reference("lattice, shuffled", 0), reference("lattice, shuffled", 1)
    assert (k5["open"] == 4).sum() == 25 and k5["boundary"] == 49 and (k9["open"] == 0).sum() == 25 and k9["boundary"] == 24
    run_case(eng, "lattice, shuffled")
    p, N = br.lattice7()   # and in lattice order, against the pinned patterns themselves
    eng.set_frames([p], [N])
    assert (eng.boundary(0, 5, 0.0, 0.0)["open"].reshape(7, 7) == br.LATTICE_K5).all() and (eng.boundary(0, 9, 0.0, 0.0)["open"].reshape(7, 7) == br.LATTICE_K9).all()


def test_duplicated_and_collinear(eng):
    d5, d30 = reference("duplicated", 0), reference("duplicated", 2)
    assert (d5["valid"] == 0).all() and d5["boundary"] == 0 and 0 < d30["boundary"] < 720
    run_case(eng, "duplicated")
    assert reference("collinear", 0)["boundary"] == 300
    run_case(eng, "collinear")


def test_normal_lengths_and_undecided_points(eng):
    nl = reference("normal lengths", 0)
    assert (nl["valid"][2::4] == 0).all() and (nl["valid"][3::4] == 0).all() and 0 < nl["flag"][0::4].sum() < 200 and 0 < nl["flag"][1::4].sum() < 200
    run_case(eng, "normal lengths")


def test_scale_and_offset(eng):
    assert 0 < reference("scale 1e-3 at 1e3", 0)["boundary"] < 800
    run_case(eng, "scale 1e-3 at 1e3")


def test_hybrid_rows(eng):
    h = reference("hybrid rows", 0)
    assert sorted(set(h["used"].tolist())) == list(range(1, 9)) and 0 < h["boundary"] < 800 and (h["valid"][h["used"] < 3] == 0).all()
    run_case(eng, "hybrid rows")


def test_small_n(eng):
    cs = br.cases()
    eng.set_frames([cs["n = %d" % m][0] for m in range(4)], [cs["n = %d" % m][1] for m in range(4)])
    for m in range(4):
        p, N, runs = cs["n = %d" % m]
        want = reference("n = %d" % m, 0)
        assert want["boundary"] == (3 if m == 3 else 0)
        check(eng, p, N, want, runs[0], "n = %d" % m, frame=m)
    got = eng.boundary(0, 3, device=True)
    assert got["flag"].shape == (0,) and got["boundary"] == 0 and eng.boundary_select(False, device=True)["xyz"].shape == (0, 3)


def test_source_1_and_a_frame_without_stored_normals(eng):
    """source 1 reads the last estimate of the frame: after estimate_normals and after fit_normals; the selections then carry no normals,
    because the frame stores none."""
    p = br.cases()["hybrid rows"][0]
    eng.set_frames([p], None)
    with pytest.raises(mvicp.MvicpError, match="status -3"):
        eng.boundary(0, 16, source=0)
    with pytest.raises(mvicp.MvicpError, match="status -3"):
        eng.boundary(0, 16, source=1)
    for est in (lambda: eng.estimate_normals(0, 12, 0.0, (0.0, 0.0, 5.0)), lambda: eng.fit_normals(0, 16, 0.0, (0.0, 0.0, 5.0), 2)):
        N = np.ascontiguousarray(est()["nrm"])
        want = br.boundary(p, N, 16, 0.0, -0.5)
        assert 0 < want["boundary"] < len(p)
        check(eng, p, None, want, (16, 0.0, -0.5), "source 1", source=1)
    # the estimate is for frame 0: another frame has none
    eng.set_frames([p, p[:100]], None)
    eng.estimate_normals(0, 12)
    with pytest.raises(mvicp.MvicpError, match="status -3"):
        eng.boundary(1, 16, source=1)


def test_device_upload(eng):
    p, N, runs = br.cases()["e2e dst"]
    eng.set_frames_device([_dev(p)], [_dev(N)])
    check(eng, p, N, reference("e2e dst", 0), runs[0], "device upload")


def test_the_search_is_left_as_the_last_neighbour_search(eng):
    p, N, _ = br.cases()["scale 1e-3 at 1e3"]
    eng.set_frames([p], [N])
    eng.boundary(0, 16)
    m, k = len(p), 16
    cnt, idx = np.zeros(m, np.int32), np.zeros((m, k), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert eng.lib.mvicp_knn_fetch(eng.h, m, m * k, vp(cnt), None, vp(idx), None) == 0
    want = reference("scale 1e-3 at 1e3", 0)["knn"]
    assert cnt.tobytes() == want["cnt"].tobytes() and idx.tobytes() == want["idx"].tobytes()


def test_history_neutral():
    pb = synth.make_problem(4, 3000)

    def run(with_boundary):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"])
            if with_boundary:
                e.boundary(2, 16)   # before the graph exists
                e.boundary_select(False)
            e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(3):
                if with_boundary:
                    e.boundary(r, 30)
                counts, weights = e.correspond(poses, pb["fixed"], 0.05)
                if with_boundary:
                    e.boundary(3 - r, 8, 0.05, 0.0, device=(r == 2))
                    e.boundary_select(r == 0, device=(r == 2))
                triples, offsets = e.map_correspondences()
                blocks = e.linearize(poses, True, True)
                if with_boundary:
                    e.boundary_select(True)
                poses, sm = e.optimize(poses, pb["fixed"])
                out.append((counts.tobytes(), weights.tobytes(), triples.tobytes(), offsets.tobytes(), np.asarray(blocks).tobytes(), poses.tobytes(),
                            sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_state_and_errors(eng):
    p, N, _ = br.cases()["hybrid rows"]
    args = (16, 0.0, -0.5)
    want = br.boundary(p, N, *args)
    assert 0 < want["boundary"] < len(p)
    fresh = mvicp.Engine(0)
    try:
        lib, h = fresh.lib, fresh.h
        bnd, fetch, select, kept = lib.mvicp_boundary, lib.mvicp_boundary_fetch, lib.mvicp_boundary_select, lib.mvicp_boundary_fetch_kept
        assert fetch(h, 10, None, None, None, None) == ERR_STATE and select(h, 1) == ERR_STATE and kept(h, 10, None, None, None) == ERR_STATE   # before any call
        assert bnd(h, 0, 0, *args) == ERR_ARG                                                     # frames not declared: out of range
        assert lib.mvicp_set_num_frames(h, 3) == 0
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.mvicp_set_frame(h, 0, dp(p), dp(N), len(p)) == 0
        assert bnd(h, 1, 0, *args) == ERR_STATE and b"never uploaded" in lib.mvicp_last_error()
        assert bnd(h, 0, 0, *args) == want["boundary"]
        n = len(p)
        flag, opn, valid, used = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)

        def result_is_still_there():
            flag[:] = 9; opn[:] = -9; valid[:] = -9; used[:] = -9
            assert fetch(h, n, vp(flag), vp(opn), vp(valid), vp(used)) == 0
            assert br.same({"flag": flag, "open": opn, "valid": valid, "used": used, "boundary": int(flag.sum())}, want)

        result_is_still_there()
        assert kept(h, n, None, None, None) == ERR_STATE and b"select" in lib.mvicp_last_error()   # a result, but no selection yet
        # refused calls keep the earlier result: every argument error is decided before the context is touched
        for bad in ((0, -1, 16, 0.0, -0.5), (0, 2, 16, 0.0, -0.5), (0, 0, 2, 0.0, -0.5), (0, 0, 65, 0.0, -0.5), (0, 0, 16, float("nan"), -0.5),
                    (0, 0, 16, float("inf"), -0.5), (0, 0, 16, 0.0, -1.0), (0, 0, 16, 0.0, 1.0), (0, 0, 16, 0.0, float("nan")), (3, 0, 16, 0.0, -0.5),
                    (-1, 0, 16, 0.0, -0.5)):
            assert bnd(h, *bad) == ERR_ARG, bad
            result_is_still_there()
        assert bnd(None, 0, 0, *args) == ERR_ARG
        # a frame never uploaded, a missing normal source: MVICP_ERR_STATE, and the result stays as well
        assert bnd(h, 2, 0, *args) == ERR_STATE
        result_is_still_there()
        assert bnd(h, 0, 1, *args) == ERR_STATE and b"estimate" in lib.mvicp_last_error()
        result_is_still_there()
        assert lib.mvicp_set_frame(h, 1, dp(p), None, n) == 0
        assert bnd(h, 1, 0, *args) == ERR_STATE and b"normals" in lib.mvicp_last_error()
        result_is_still_there()
        ws = br.select(p, N, want, True)
        assert 0 < ws["kept"] < n and select(h, 1) == ws["kept"]
        xyz, nrm, idx = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
        assert kept(h, ws["kept"] - 1, vp(xyz), None, None) == ERR_ARG                            # cap < kept
        assert fetch(h, n - 1, vp(flag), None, None, None) == ERR_ARG
        assert kept(h, ws["kept"], vp(xyz), vp(nrm), vp(idx)) == 0
        m = ws["kept"]
        assert xyz[:m].tobytes() == ws["xyz"].tobytes() and nrm[:m].tobytes() == ws["nrm"].tobytes() and idx[:m].tobytes() == ws["idx"].tobytes()
        # an upload to another slot leaves the result, an upload to its frame ends it; so does mvicp_set_num_frames
        assert lib.mvicp_set_frame(h, 2, dp(p), dp(N), n) == 0
        result_is_still_there()
        assert lib.mvicp_set_frame(h, 0, dp(p), None, n) == 0
        assert fetch(h, n, vp(flag), None, None, None) == ERR_STATE and select(h, 1) == ERR_STATE and kept(h, n, None, None, None) == ERR_STATE
        # a frame without stored normals, by the estimate: the selection carries none
        assert lib.mvicp_estimate_normals(h, 0, 12, 0.0, None) == n and bnd(h, 0, 1, *args) >= 0 and select(h, 0) >= 0
        assert kept(h, n, vp(xyz), vp(nrm), None) == ERR_STATE and b"normals" in lib.mvicp_last_error()
        assert kept(h, n, vp(xyz), None, None) == 0
        assert lib.mvicp_set_num_frames(h, 1) == 0 and fetch(h, 1 << 20, None, None, None, None) == ERR_STATE
    finally:
        fresh.close()
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        eng.boundary(0, 30, 0.0, 1.0)
