"""No GPU: tests/rejectref.py (the masked search in numpy) pinned on hand-made lists; the registration the masked search is for -- the 25-round
host loop of tests/test_boundary_cpu.py with the edge's scale taken over the KEPT pairs, as mvicp_set_reject_mask defines it -- on the partial
and the full pair, point-to-plane and symmetric; and the new entry points' declarations and GPU-free refusals."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import boundref as br
import matchref
import mvicp
import rejectref
import symref
import test_boundary_cpu
import test_sym_cpu
from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("mvicp_set_reject_mask", "mvicp_boundary_adopt", "mvicp_get_reject_mask")


def _w(d):
    return np.float32(1.5 * d)


def test_rejectref_on_hand_made_lists():
    first = np.array([0, 1, 2, 4, 5, 7], dtype=np.int32)
    second = np.array([3, 3, 0, 1, 2, 6], dtype=np.int32)
    dist = np.array([0.5, 0.1, 0.4, 0.2, 0.3, 0.6])
    src = np.zeros(8, dtype=np.uint8); dst = np.zeros(7, dtype=np.uint8)
    # no mask: even length 6 -> the UPPER median, sorted[3] = 0.4
    f, s, d, w = rejectref.masked(first, second, dist, None, None)
    assert f.tobytes() == first.tobytes() and s.tobytes() == second.tobytes() and d.tobytes() == dist.tobytes()
    assert w.dtype == np.float32 and w == _w(0.4)
    # all-zero masks equal no mask
    f, s, d, w = rejectref.masked(first, second, dist, src, dst)
    assert f.tobytes() == first.tobytes() and w == _w(0.4)
    # source mask only: query 2 goes -> odd length 5, sorted = .1 .2 .3 .5 .6 -> 0.3
    src[2] = 1
    f, s, d, w = rejectref.masked(first, second, dist, src, None)
    assert f.tolist() == [0, 1, 4, 5, 7] and s.tolist() == [3, 3, 1, 2, 6] and d.tolist() == [0.5, 0.1, 0.2, 0.3, 0.6] and w == _w(0.3)
    # target mask only: target 3 is the neighbour of two queries, both go (neither is re-matched) -> even length 4, sorted = .2 .3 .4 .6 -> 0.4
    dst[3] = 7   # (any nonzero byte rejects)
    f, s, d, w = rejectref.masked(first, second, dist, None, dst)
    assert f.tolist() == [2, 4, 5, 7] and s.tolist() == [0, 1, 2, 6] and d.tolist() == [0.4, 0.2, 0.3, 0.6] and w == _w(0.4)
    # both: .2 .3 .6 -> 0.3
    f, s, d, w = rejectref.masked(first, second, dist, src, dst)
    assert f.tolist() == [4, 5, 7] and d.tolist() == [0.2, 0.3, 0.6] and w == _w(0.3)
    # a flag on a point no pair touches changes nothing
    src2 = np.zeros(8, dtype=np.uint8); src2[3] = src2[6] = 1
    assert rejectref.masked(first, second, dist, src2, None)[0].tobytes() == first.tobytes()
    # an empty kept list: weight 0, empty arrays of the right types
    f, s, d, w = rejectref.masked(first, second, dist, np.ones(8, dtype=np.uint8), None)
    assert len(f) == len(s) == len(d) == 0 and f.dtype == np.int32 and s.dtype == np.int32 and d.dtype == np.float64 and w == np.float32(0) and w.dtype == np.float32
    f, s, d, w = rejectref.masked(first[:0], second[:0], dist[:0], src, dst)
    assert len(f) == 0 and w == np.float32(0)
    # one pair: the median is that pair
    assert rejectref.masked(first[:1], second[:1], dist[:1], None, None)[3] == _w(0.5)
    # ties at the median: the value is the tied one whichever copy the sort puts there, even and odd
    tied = np.array([0.25, 0.5, 0.25, 0.25, 0.75, 0.1])
    assert rejectref.masked(first, second, tied, None, None)[3] == _w(0.25)         # sorted .1 .25 .25 .25 .5 .75 -> [3] = .25
    src3 = np.zeros(8, dtype=np.uint8); src3[7] = 1
    assert rejectref.masked(first, second, tied, src3, None)[3] == _w(0.25)         # .25 .25 .25 .5 .75 -> [2] = .25
    src3[0] = 1
    assert rejectref.masked(first, second, tied, src3, None)[3] == _w(0.5)          # .25 .25 .5 .75 -> [2] = .5: the upper of the two middle ones
    with pytest.raises(ValueError):
        rejectref.masked(first, second, dist[:3], None, None)


def searched(src, Ps, dst, Pd, cutoff):
    """symref.nn_cutoff with the kept distances: -> (first, second, dist, a)"""
    Rel = np.linalg.inv(Pd) @ Ps
    x = src @ Rel[:3, :3].T + Rel[:3, 3]
    d2 = ((x[:, None, :] - dst[None, :, :]) ** 2).sum(-1)
    j = np.argmin(d2, axis=1)
    d = np.sqrt(d2[np.arange(len(src)), j])
    keep = d < float(np.float32(cutoff))
    first, second, dist = np.nonzero(keep)[0].astype(np.int32), j[keep].astype(np.int32), d[keep]
    a = np.float32(1.5 * np.sort(dist)[len(dist) // 2]) if len(dist) else np.float32(0)
    return first, second, dist, a


def masked_registration(cl, symmetric, dst_mask, cutoff_spacings=3.0, rounds=25):
    """test_boundary_cpu.boundary_registration with the edge's scale taken over the KEPT pairs (rejectref.masked): what a registration with
    mvicp_set_reject_mask(target, mask, AS_TARGET) set once before the loop computes -> final pose of src"""
    src, dst, sn, dn = cl["src"], cl["dst"], cl["src_nrm"], cl["dst_nrm"]
    P = np.array([np.eye(4), symref.start_pose(cl["truth"], cl["spacing"])])
    for rnd in range(rounds):
        first, second, dist, a_all = searched(src, P[1], dst, P[0], cutoff_spacings * cl["spacing"])
        if rnd == 0:   # (the search above is the suite's own)
            f0, s0, a0 = symref.nn_cutoff(src, P[1], dst, P[0], cutoff_spacings * cl["spacing"])
            assert f0.tobytes() == first.tobytes() and s0.tobytes() == second.tobytes() and a0 == a_all
        first, second, _, a = rejectref.masked(first, second, dist, None, dst_mask)
        p, q, nq, npn = src[first], dst[second], dn[second], sn[first]

        def evaluate(poses):
            if symmetric:
                return symref.blocks_fp64(p, q, nq, npn, poses[1], poses[0], a, True)[None, :]
            return test_sym_cpu._plane_fp64(p, q, nq, poses[1], poses[0], a, True)[None, :]

        P, _ = L.lm_solve_host(2, [1], [0], P, [1, 0], L.PARAM_SOPHUS_SE3, evaluate, 50)
    return P[1]


@functools.lru_cache(maxsize=None)
def masked_figures(partial, symmetric):
    """-> (deg, spacings) of the registration with the target's boundary mask at (30, -0.5) inside the search"""
    cl = matchref.e2e_clouds(partial)
    mask = br.boundary(cl["dst"], cl["dst_nrm"], 30, 0.0, -0.5)["flag"]
    return symref.distance_to_truth(masked_registration(cl, symmetric, mask), cl["truth"], cl["src"], cl["spacing"])


# This run, (partial, symmetric) -> (deg, spacings) with the scale over the kept pairs; "none" and "scale as searched" are
# test_boundary_cpu.registration_figures.  tests/test_gpu_reject_mask.py asserts the partial pair's to these four digits.
FIGURES = {(True, False): ("0.0469", "0.0713"), (True, True): ("0.0017", "0.0032"), (False, False): ("0.0306", "0.0497"), (False, True): ("0.0043", "0.0061")}
# the combinations in which this run ends closer to the truth than no rejection, in rotation AND in displacement: all four
# (none: 0.0817 / 0.1091, 0.0041 / 0.0083, 0.0315 / 0.0549, 0.0045 / 0.0063; scale as searched: 0.0467 / 0.0716, then as above)
CLOSER = {(True, False), (True, True), (False, False), (False, True)}


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("partial", [True, False])
def test_registration_with_the_scale_over_the_kept_pairs(partial, symmetric):
    none, as_searched = test_boundary_cpu.registration_figures(partial, symmetric)
    got = masked_figures(partial, symmetric)
    print("partial=%s symmetric=%s  none %.4f deg, %.4f spacings | scale as searched %.4f, %.4f | scale over the kept pairs %.4f, %.4f" % (
        (partial, symmetric) + none + as_searched + got))
    assert ("%.4f" % got[0], "%.4f" % got[1]) == FIGURES[(partial, symmetric)]
    closer = got[0] < none[0] and got[1] < none[1]
    assert closer == ((partial, symmetric) in CLOSER), (none, got)


def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    assert re.search(r"MVICP_REJECT_AS_TARGET\s*=\s*1\b", txt) and re.search(r"MVICP_REJECT_AS_SOURCE\s*=\s*2\b", txt)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)
    for name in ("set_reject_mask", "adopt_boundary_mask", "reject_mask", "reject_correspondences"):
        assert hasattr(mvicp.Engine, name)
    assert (L.REJECT_AS_TARGET, L.REJECT_AS_SOURCE) == (1, 2)


def test_argument_errors_need_no_gpu(engine_lib):
    set_mask, adopt, get = engine_lib.mvicp_set_reject_mask, engine_lib.mvicp_boundary_adopt, engine_lib.mvicp_get_reject_mask
    byte = C.create_string_buffer(8)
    assert set_mask(None, 0, byte, 1) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert adopt(None, 1) == ERR_ARG and get(None, 0, None, 0, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context (no frames, no boundary result)
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    for roles in (-1, 4, 7):
        assert set_mask(ctx, 0, byte, roles) == ERR_ARG and b"roles" in engine_lib.mvicp_last_error(), roles
        assert adopt(ctx, roles) == ERR_ARG and b"roles" in engine_lib.mvicp_last_error(), roles
    for frame in (0, -1, 5):
        for roles in (0, 1, 2, 3):
            assert set_mask(ctx, frame, byte, roles) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), (frame, roles)
        assert set_mask(ctx, frame, None, 1) == ERR_ARG
        r = C.c_int(9)
        assert get(ctx, frame, None, 0, C.byref(r)) == ERR_ARG and r.value == 9
    assert fake.raw == bytes(1 << 16)
