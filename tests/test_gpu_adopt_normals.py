"""mvicp_normals_adopt on the MI355X: after adoption the frame behaves, byte for byte, like a frame uploaded with the contract's normals
(tests/normref.py) -- the PLANE and SYMMETRIC blocks of mvicp_linearize_metric equal those of a twin engine uploaded with them, whether
the adoption comes before the first search, between a search and a solve (the lists are re-gathered) or into a frame uploaded without
normals; mvicp_fpfh reads them; refusals change nothing; mvicp_recompute_normals still gives its old bytes afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import fpfhref
import mvicp
import normref
from mvicp import synth
from mvicp.lib import METRIC_PLANE, METRIC_SYMMETRIC, MvicpError

pytestmark = pytest.mark.gpu

K, VIEW = 16, (0.0, 0.0, 2.0)


@functools.lru_cache(maxsize=None)
def world():
    """-> (problem of three clouds of 1500 points, the contract's normals of each)"""
    pb = synth.make_problem(3, 1500)
    return pb, [normref.normals(p, K, 0.0, VIEW)["nrm"] for p in pb["pts"]]


def blocks(e, pb):
    return tuple(np.asarray(e.linearize_metric(pb["init"], m, True)).tobytes() for m in (METRIC_PLANE, METRIC_SYMMETRIC))


@functools.lru_cache(maxsize=None)
def twin_blocks():
    """what an engine uploaded with the contract's normals computes"""
    pb, nrm = world()
    e = mvicp.Engine(0)
    try:
        e.set_frames(pb["pts"], nrm); e.set_graph(pb["src"], pb["dst"])
        e.correspond(pb["init"], pb["fixed"], 0.05)
        return blocks(e, pb)
    finally:
        e.close()


def adopt_all(e, pb, nrm):
    for i in range(len(pb["pts"])):
        got = e.estimate_normals(i, K, 0.0, VIEW)
        assert got["nrm"].tobytes() == nrm[i].tobytes()
        e.adopt_normals()
        out = np.zeros_like(nrm[i])   # (the result stays fetchable after adoption)
        assert e.lib.mvicp_normals_fetch(e.h, len(out), out.ctypes.data_as(C.c_void_p), None, None) == 0 and out.tobytes() == nrm[i].tobytes()


@pytest.mark.parametrize("case", ["before the first search", "between a search and a solve", "a frame uploaded without normals"])
def test_adopted_normals_are_the_frames_normals(case):
    pb, nrm = world()
    e = mvicp.Engine(0)
    try:
        e.set_frames(pb["pts"], None if case.startswith("a frame") else pb["nor"])
        if case == "before the first search":
            adopt_all(e, pb, nrm)
            e.set_graph(pb["src"], pb["dst"])
            e.correspond(pb["init"], pb["fixed"], 0.05)
        else:
            e.set_graph(pb["src"], pb["dst"])
            e.correspond(pb["init"], pb["fixed"], 0.05)
            if case.startswith("a frame"):
                with pytest.raises(MvicpError):
                    e.linearize_metric(pb["init"], METRIC_PLANE, True)
            else:
                assert blocks(e, pb) != twin_blocks()
            adopt_all(e, pb, nrm)
        assert blocks(e, pb) == twin_blocks()
        for i in range(3):
            assert e.get_structure(i, "snor").view(np.float64).reshape(-1, 3)[e.get_structure(i, "inv").view(np.int32)].tobytes() == nrm[i].tobytes()
        # the next round (lists unchanged, so they would be reused) still sees the adopted normals, and so does a solve
        e.correspond(pb["init"], pb["fixed"], 0.05)
        assert blocks(e, pb) == twin_blocks()
    finally:
        e.close()


def test_a_solve_after_adoption_equals_the_twins():
    pb, nrm = world()

    def run(adopt):
        e = mvicp.Engine(0)
        try:
            e.set_frames(pb["pts"], pb["nor"] if adopt else nrm); e.set_graph(pb["src"], pb["dst"])
            poses, out = pb["init"].copy(), []
            for r in range(2):
                e.correspond(poses, pb["fixed"], 0.05)
                if adopt and r == 0:
                    adopt_all(e, pb, nrm)      # voids the evaluation the search queued
                poses, sm = e.optimize_metric(poses, pb["fixed"])
                out.append((poses.tobytes(), sm["iterations"], sm["final_cost"]))
            return out
        finally:
            e.close()

    assert run(True) == run(False)


def test_fpfh_reads_the_adopted_normals():
    pb, nrm = world()
    e = mvicp.Engine(0)
    try:
        e.set_frames(pb["pts"][:1], None)
        with pytest.raises(MvicpError):
            e.fpfh(0, 0.08, 32)
        e.estimate_normals(0, K, 0.0, VIEW); e.adopt_normals()
        got, want = e.fpfh(0, 0.08, 32), fpfhref.fpfh(pb["pts"][0], nrm[0], 0.08, 32)
        assert (want["used"] > 0).sum() > 1000
        assert got["desc"].tobytes() == want["desc"].tobytes() and got["used"].tobytes() == want["used"].tobytes()
    finally:
        e.close()


def test_refused_adoptions_change_nothing_and_recompute_normals_keeps_its_bytes():
    pb, nrm = world()
    e = mvicp.Engine(0)
    try:
        e.set_frames(pb["pts"], pb["nor"])
        old = [e.recompute_normals(i, 10) for i in range(3)]
        with pytest.raises(MvicpError):
            e.adopt_normals()                                  # no result
        e.estimate_normals(1, K, 0.0, VIEW)
        e.set_frame(1, pb["pts"][1], pb["nor"][1])            # uploaded again: the result is dropped
        with pytest.raises(MvicpError) as ei:
            e.adopt_normals()
        assert "status -3" in str(ei.value)
        assert e.lib.mvicp_normals_fetch(e.h, 1 << 20, None, None, None) == -3
        stored = e.get_structure(1, "snor").view(np.float64).reshape(-1, 3)[e.get_structure(1, "inv").view(np.int32)]
        assert stored.tobytes() == np.ascontiguousarray(pb["nor"][1]).tobytes()
        e.estimate_normals(0, K, 0.0, VIEW)
        e.set_frame(1, pb["pts"][1], pb["nor"][1])            # an upload to ANOTHER frame leaves the result
        e.adopt_normals()
        e.estimate_normals(2, K, 0.0, VIEW); e.adopt_normals()
        for i in range(3):
            assert e.recompute_normals(i, 10).tobytes() == old[i].tobytes()
    finally:
        e.close()
