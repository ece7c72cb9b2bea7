"""The contract of mvicp_segment_plane on the CPU: tests/planeref.py's numpy form equals its scalar loop on every generator;
mvicp_plane_from_moments through the C ABI equals the reference's refit rule byte for byte (moments of every generator, synthetic moments
at b = 20 and b = 15, 128-bit values exactly halfway between two doubles); the refit is a plane fit (against numpy.linalg.eigh, under the
bar derived in DESIGN.md section 3.19); the argument errors need no GPU."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import clusterref
import mvicp
import planeref as pr
from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
NAMES = ("mvicp_segment_plane", "mvicp_plane_fetch", "mvicp_plane_select", "mvicp_plane_fetch_kept", "mvicp_plane_from_moments")


@functools.lru_cache(maxsize=None)
def clouds():
    """name -> (points, tau, the argument sets (H, seed, axis, cos_min) to run); sizes the scalar loop gets through in a second or two"""
    noisy = pr.noisy_plane_cloud()[0]
    fw = pr.floor_wall_cloud()[0]
    return {
        "noisy plane": (noisy[:700], pr.NOISY_TAU, ((24, 0, None, 0.0), (24, 7, None, 0.0))),
        "dyadic slab, tau = pitch / 4": (pr.dyadic_slab(), pr.SLAB_PITCH / 4, ((32, 0, None, 0.0),)),
        "dyadic slab, tau = pitch": (pr.dyadic_slab(), pr.SLAB_PITCH, ((32, 0, None, 0.0), (32, 0, (0.0, 0.0, -3.0), 1.0))),
        "floor + wall": (fw[:800], pr.FLOOR_WALL_TAU, ((32, 0, None, 0.0), (64, 0, (0.0, 0.0, 2.0), 0.9), (16, 3, (1.0, 0.0, 0.0), 0.0))),
        "tabletop": (pr.tabletop_cloud()[0][:800], pr.TABLE_TAU, ((24, 0, None, 0.0),)),
        "line": (pr.line_cloud()[:200], 0.01, ((32, 0, None, 0.0),)),
        "every point twice": (np.repeat(noisy[:150], 2, axis=0), pr.NOISY_TAU, ((48, 0, None, 0.0),)),
        "at 1e200": (np.full((100, 3), 1e200) + np.arange(300.0).reshape(100, 3) * 1e185, 0.01, ((24, 0, None, 0.0),)),
        "far off the origin": (noisy[:500] + 4e6, pr.NOISY_TAU, ((24, 0, None, 0.0),)),
        "n = 2": (noisy[:2], 0.01, ((16, 0, None, 0.0),)),
        "n = 3": (noisy[:3], 0.01, ((16, 0, None, 0.0),)),
    }


@pytest.mark.parametrize("name", sorted(clouds()))
def test_numpy_form_equals_the_scalar_loop(name):
    p, tau, runs = clouds()[name]
    for H, seed, axis, cos_min in runs:
        for refine in (True, False):
            got = pr.segment(p, None, tau, H, seed, axis, cos_min, refine)
            want = pr.segment_loop(p, None, tau, H, seed, axis, cos_min, refine)
            assert pr.same(got, want), (name, H, seed, axis, refine, {k: (got[k], want[k]) for k in pr.RECORD_INTS})
            assert got["refit"] == (1 if refine and got["best"] >= 0 and got["count"] > 1 else 0) or name == "every point twice"
            assert int(got["flags"].sum()) == got["count_refined"] and (got["counts"] >= 0).sum() == got["accepted"]
            for inliers in (True, False):
                sel = pr.select(p, None, got, inliers)
                assert (np.diff(sel["idx"]) > 0).all() and sel["xyz"].tobytes() == p[sel["idx"]].tobytes()
    if name in ("line", "at 1e200", "n = 2"):
        assert got["accepted"] == 0 and got["best"] == -1 and not got["flags"].any()
    elif name != "n = 3":
        assert got["accepted"] > 0 and got["count"] >= 3


def _abi(lib, c, s, S, q, a, m):
    s = np.array([int(v) for v in s], dtype=np.int64); S = np.array([int(v) for v in S], dtype=np.int64)
    a = np.ascontiguousarray(a, dtype=np.float64); m = np.ascontiguousarray(m, dtype=np.float64)
    out = np.full(8, 7.0)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    st = lib.mvicp_plane_from_moments(int(c), vp(s), vp(S), int(q), dp(a), dp(m), dp(out[:3]), dp(out[4:7]))
    assert out[3] == 7.0 and out[7] == 7.0
    return st, out[:3].copy(), out[4:7].copy()


def _equal(lib, c, s, S, q, a, m):
    st, nv, g = _abi(lib, c, s, S, q, a, m)
    wn, wg = pr.from_moments(c, s, S, q, a, m)
    assert st == 0 and nv.tobytes() == wn.tobytes() and g.tobytes() == wg.tobytes(), (c, s, S, q, nv, wn, g, wg)
    pn, pg = mvicp.plane_from_moments(c, s, S, q, a, m)
    assert pn.tobytes() == wn.tobytes() and pg.tobytes() == wg.tobytes()
    assert abs(float(np.linalg.norm(nv)) - 1.0) < 1e-15
    return nv, g


def test_from_moments_on_the_moments_of_every_generator(engine_lib):
    done = 0
    for name, (cloud, tau) in {"noisy": (pr.noisy_plane_cloud()[0], pr.NOISY_TAU), "slab / 4": (pr.dyadic_slab(), pr.SLAB_PITCH / 4),
                               "slab": (pr.dyadic_slab(), pr.SLAB_PITCH), "floor + wall": (pr.floor_wall_cloud()[0], pr.FLOOR_WALL_TAU),
                               "tabletop": (pr.tabletop_cloud()[0], pr.TABLE_TAU), "far": (pr.noisy_plane_cloud()[0] + 4e6, pr.NOISY_TAU)}.items():
        for H, seed in ((64, 0), (64, 11), (8, 5)):
            r = pr.segment(cloud, None, tau, H, seed)
            assert r["refit"] == 1 and r["b"] == 21, name
            nv, g = _equal(engine_lib, *r["moments"])
            assert nv.tobytes() == r["normal"].tobytes() and g.tobytes() == r["point"].tobytes()
            done += 1
    assert done == 18
    assert pr.segment(pr.line_cloud(), None, 0.01, 64, 0)["moments"] is None   # (nothing accepted: nothing to refit)


def _synthetic(c, b, seed):
    """The exact sums of c integer points: 1024 distinct vectors below 2^b on a thin slab, each c / 1024 times."""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = rng.integers(-(1 << b), 1 << b, size=(1024, 3), dtype=np.int64)
    M[:, 2] = rng.integers(-(1 << (b - 9)), 1 << (b - 9), size=1024)
    rep = c // 1024
    s = [rep * int(M[:, k].sum()) for k in range(3)]
    S = [rep * int((M[:, k] * M[:, l]).sum()) for k in range(3) for l in range(k, 3)]
    return s, S


@pytest.mark.parametrize("c,b", [(1 << 20, 20), (1 << 30, 15)])
def test_from_moments_at_the_bit_budgets_of_large_sets(engine_lib, c, b):
    assert pr.bit_rule(c, 0.7)[0] == b and pr.bit_rule(c - 1, 0.7)[0] == (16 if b == 15 else 21)   # the budget steps down exactly at c
    for seed in (1, 2, 3):
        s, S = _synthetic(c, b, seed)
        assert all(abs(v) < 1 << (c.bit_length() + b) for v in s) and all(abs(v) < 1 << 62 for v in S)   # the contract's bounds
        assert max(c * v for v in S[0:1]).bit_length() > 64                                                # a 128-bit product indeed
        q = pr.bit_rule(c, 0.7)[1]
        nv, g = _equal(engine_lib, c, s, S, q, (0.25, -1.5, 3.0), (0.0, 0.0, -1.0))
        assert nv[2] < -0.99                                                                              # the slab's normal, turned to m


def _halfway_sets():
    """Two sets of 255 integers below 2^20 whose c S_00 - s_0^2 needs 55 bits and ends in binary 10: exactly halfway between two doubles,
    one with an even lower neighbour (the tie goes down) and one with an odd (it goes up).  (An odd c: with an even one the value is
    never 2 mod 4.)"""
    rng = np.random.Generator(np.random.PCG64(55))
    found = {}
    while len(found) < 2:
        M = rng.integers(-(1 << 20), 1 << 20, size=(255, 3), dtype=np.int64)
        V = 255 * int((M[:, 0] * M[:, 0]).sum()) - int(M[:, 0].sum()) ** 2
        if V.bit_length() == 55 and V % 4 == 2:
            found.setdefault((V >> 2) & 1, M)
    return found


def test_from_moments_rounds_a_halfway_value_to_even(engine_lib):
    for low_bit, M in sorted(_halfway_sets().items()):
        c = len(M)
        s = [int(M[:, k].sum()) for k in range(3)]
        S = [int((M[:, k] * M[:, l]).sum()) for k in range(3) for l in range(k, 3)]
        V = c * S[0] - s[0] * s[0]
        assert V.bit_length() == 55 and V % 4 == 2 and float(V) != V            # spacing 4 at 2^54: V lies on the midpoint
        assert int(float(V)) == (V - 2 if low_bit == 0 else V + 2)             # nearest even, in both directions
        assert int(np.nextafter(float(V), 0.0)) != V and (int(float(V)) >> 2) % 2 == 0
        _equal(engine_lib, c, s, S, 20, (1.0, 2.0, 3.0), (0.0, 0.0, 1.0))


def test_from_moments_argument_errors(engine_lib):
    s, S = [3, 0, -3], [5, 0, -5, 2, 0, 5]
    a, m = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    assert _abi(engine_lib, 3, s, S, 4, a, m)[0] == 0
    for c in (0, -1, 1 << 31):
        assert _abi(engine_lib, c, s, S, 4, a, m)[0] == ERR_ARG and b"2^31" in engine_lib.mvicp_last_error()
    for q in (-1101, 1101):
        assert _abi(engine_lib, 3, s, S, q, a, m)[0] == ERR_ARG and b"q =" in engine_lib.mvicp_last_error()
    for bad in (float("nan"), float("inf")):
        assert _abi(engine_lib, 3, s, S, 4, (bad, 0.0, 0.0), m)[0] == ERR_ARG and _abi(engine_lib, 3, s, S, 4, a, (0.0, bad, 0.0))[0] == ERR_ARG
    assert _abi(engine_lib, 3, s, [-1, 0, 0, 2, 0, 5], 4, a, m)[0] == ERR_ARG                    # a negative sum of squares
    assert _abi(engine_lib, 3, [9, 0, 0], S, 4, a, m)[0] == ERR_ARG and b"one set" in engine_lib.mvicp_last_error()   # 3 * 5 - 81 < 0
    ok = np.zeros(3); i3 = np.zeros(3, np.int64); i6 = np.zeros(6, np.int64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    full = [1, vp(i3), vp(i6), 0, dp(ok), dp(ok), dp(ok), dp(ok)]
    for k in (1, 2, 4, 5, 6, 7):
        args = list(full); args[k] = None
        assert engine_lib.mvicp_plane_from_moments(*args) == ERR_ARG, k
    with pytest.raises(mvicp.MvicpError, match="status -1"):
        mvicp.plane_from_moments(0, s, S, 4, a, m)
    # one point: every C entry is zero, no rotation happens, the vector is the first axis turned to m
    st, nv, g = _abi(engine_lib, 1, [4, 4, 4], [16, 16, 16, 16, 16, 16], 2, (1.0, 1.0, 1.0), (-1.0, 0.0, 0.0))
    assert st == 0 and nv.tolist() == [-1.0, 0.0, 0.0] and g.tolist() == [2.125, 2.125, 2.125]


def _angle(u, v):
    """The angle between two unit vectors from the cross product's norm (arccos cannot resolve a small one)."""
    return math.asin(min(1.0, float(np.linalg.norm(np.cross(u, v)))))


def test_the_refit_is_a_plane_fit():
    """On noisy_plane_cloud the refined normal against numpy.linalg.eigh of the fp64 covariance of the same inliers.  The bar is the
    first-order perturbation bound of DESIGN.md section 3.19: in units of the quantisation step 2^-q the integer points differ from the
    real ones by e_i in (-1, 0]^3, whose centred second moment is at most 3 / 4, so the covariance moves by at most
    sqrt(3 tr C) + 3 / 4 in the 2-norm and the eigenvector of the smallest eigenvalue by at most that over the gap to the next one;
    2^-40 on top for the rounding of the two eigen-solvers."""
    p, _, mask = pr.noisy_plane_cloud()
    r = pr.segment(p, None, pr.NOISY_TAU, 512, 0)
    assert r["refit"] == 1 and r["b"] == 21
    hyp = np.abs(pr._residual(r["hyp_normal"][None], r["hyp_point"][None], p))[0] <= pr.NOISY_TAU
    assert int(hyp.sum()) == r["count"] == r["moments"][0]
    x = p[hyp]
    mean = x.mean(0)
    cov = (x - mean).T @ (x - mean) / len(x)
    w, V = np.linalg.eigh(cov)
    ref = V[:, 0] if V[:, 0] @ r["normal"] > 0 else -V[:, 0]
    scale = 4.0 ** r["q"]
    bar = (math.sqrt(3.0 * float(w.sum()) * scale) + 0.75) / ((w[1] - w[0]) * scale) + 2.0 ** -40
    got = _angle(r["normal"], ref)
    step = 2.0 ** -r["q"]
    print("refit against eigh: %.3e rad, bar %.3e rad; quantisation step %.3e; centroid against numpy's mean: %.4f steps"
          % (got, bar, step, float(np.abs(r["point"] - mean).max()) / step))
    assert got <= bar
    a_hyp, a_fit = _angle(r["hyp_normal"], pr.NOISY_NORMAL), _angle(r["normal"], pr.NOISY_NORMAL)
    print("from the true normal: hypothesis %.4f deg, refit %.4f deg" % (math.degrees(a_hyp), math.degrees(a_fit)))
    assert a_fit < a_hyp


def test_the_cases_hold_what_they_are_for():
    """The facts the GPU tests rely on, on the reference alone."""
    p, nr, mask = pr.noisy_plane_cloud()
    r64, r512 = pr.segment(p, nr, pr.NOISY_TAU, 64, 0), pr.segment(p, nr, pr.NOISY_TAU, 512, 0)
    assert r64["accepted"] == 64 and r512["accepted"] == 512
    assert (r64["count"], r512["count"]) == (2000, 2003) and (r512["counts"] == 2003).sum() == 1 and (r64["counts"] == 2000).sum() == 1
    assert (r512["flags"][mask] == 1).mean() > 0.99 and (r512["flags"][~mask] == 1).sum() < 40
    tt, part = pr.tabletop_cloud()
    one = clusterref.cluster(tt, None, pr.TABLE_RADIUS, pr.TABLE_MIN_PTS)
    assert one["stats"]["clusters"] == 1 and (one["label"] == 0).all()       # the floor joins the two boxes into ONE cluster
    rest = pr.select(tt, None, pr.segment(tt, None, pr.TABLE_TAU, 256, 0), False)
    two = clusterref.cluster(rest["xyz"], None, pr.TABLE_RADIUS, pr.TABLE_MIN_PTS)
    assert two["stats"]["clusters"] == 2 and two["stats"]["noise"] == 0
    assert [set(part[rest["idx"]][two["label"] == k].tolist()) for k in (0, 1)] in ([{1}, {2}], [{2}, {1}])


def test_symbols_are_declared_bound_and_exported(engine_lib):
    txt = open(os.path.join(ROOT, "include", "mvicp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in L.SYMBOLS and hasattr(engine_lib, name)
    assert hasattr(mvicp, "plane_from_moments") and hasattr(mvicp.Engine, "segment_plane") and hasattr(mvicp.Engine, "plane_select")


def test_argument_errors_need_no_gpu(engine_lib):
    seg, fetch, select, kept = engine_lib.mvicp_segment_plane, engine_lib.mvicp_plane_fetch, engine_lib.mvicp_plane_select, engine_lib.mvicp_plane_fetch_kept
    R = L.PlaneResult()
    assert seg(None, 0, 64, 0, 0.01, None, 0.0, 1, C.byref(R)) == ERR_ARG and b"null context" in engine_lib.mvicp_last_error()
    assert fetch(None, 0, None, 0, None) == ERR_ARG and select(None, 1) == ERR_ARG and kept(None, 0, None, None, None) == ERR_ARG
    # decided BEFORE the context is touched: a block of zero bytes stands in for a context, and the message names the argument
    fake = C.create_string_buffer(1 << 16)
    ctx = C.cast(fake, C.c_void_p)
    assert seg(ctx, 0, 64, 0, 0.01, None, 0.0, 1, None) == ERR_ARG and b"result" in engine_lib.mvicp_last_error()
    for H in (0, -1, (1 << 24) + 1):
        assert seg(ctx, 0, H, 0, 0.01, None, 0.0, 1, C.byref(R)) == ERR_ARG and b"hypotheses" in engine_lib.mvicp_last_error(), H
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -1.0):
        assert seg(ctx, 0, 64, 0, bad, None, 0.0, 1, C.byref(R)) == ERR_ARG and b"tau" in engine_lib.mvicp_last_error(), bad
    ax = lambda *v: (C.c_double * 3)(*v)
    for bad in (ax(0.0, 0.0, 0.0), ax(float("nan"), 0.0, 1.0), ax(0.0, float("inf"), 1.0)):
        assert seg(ctx, 0, 64, 0, 0.01, bad, 0.5, 1, C.byref(R)) == ERR_ARG and b"axis" in engine_lib.mvicp_last_error()
    for bad in (-0.1, 1.5, float("nan")):
        assert seg(ctx, 0, 64, 0, 0.01, ax(0.0, 0.0, 1.0), bad, 1, C.byref(R)) == ERR_ARG and b"cos_min" in engine_lib.mvicp_last_error(), bad
    for frame in (0, -1, 5):   # (a context without frames: every index is out of range; cos_min is not looked at without an axis)
        assert seg(ctx, frame, 64, 0, 0.01, None, 7.0, 1, C.byref(R)) == ERR_ARG and b"out of range" in engine_lib.mvicp_last_error(), frame
    assert fake.raw == bytes(1 << 16)


def test_without_a_gpu_the_call_fails_loudly(engine_lib):
    """No device, no context, no plane: mvicp_create refuses (there is no CPU path) and mvicp_segment_plane on the context it did not make
    reports an error instead of an answer.  With a device the same calls succeed on an empty context."""
    h = C.c_void_p()
    st = engine_lib.mvicp_create(0, C.byref(h))
    try:
        if st != 0:
            assert st == -2 and not h.value and b"no CPU fallback" in engine_lib.mvicp_last_error()
            with pytest.raises(mvicp.MvicpError):
                mvicp.Engine(0)
        R = L.PlaneResult()
        assert engine_lib.mvicp_segment_plane(h, 0, 64, 0, 0.01, None, 0.0, 1, C.byref(R)) == ERR_ARG   # a NULL context, or a context without frames
        assert len(engine_lib.mvicp_last_error()) > 0
    finally:
        if h.value:
            engine_lib.mvicp_destroy(h)
