"""-m gpu: accuracy of mvicp_recompute_normals (csrc/normals.hip: k-NN, covariance, cyclic Jacobi) judged on EVERY point — degenerate
neighbourhoods included — by the Rayleigh residual of the returned normal on the long-double covariance of the kernel's own k-NN set
(tests/normcheck.py; bar: 32 x numpy's own fp64 route on the same sets, floored at 2^-52), over scales, offsets and degenerate shapes.

No cloud here has isolated points far from the rest: the kernel's ring growth scans (2r+1)^3 cells per step, a known limit."""
import numpy as np
import pytest

import mvicp
import normcheck
from mvicp.lib import MvicpError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


def _cloud(rng, n, kind):
    """the kinds of test_random_shapes_knn_lists_equal_nanoflann, extent ~ 1"""
    if kind == "blob":
        return rng.normal(0.0, 0.25, (n, 3))
    if kind == "plane":      # tilted, so the plane is not exact in fp64
        uv = rng.uniform(-1, 1, (n, 2))
        return uv @ np.array([[0.8, 0.1, 0.3], [-0.2, 0.9, 0.25]])
    if kind == "lattice":    # range-image grid: exact ties, with a smooth quantised depth
        side = int(np.ceil(n ** 0.5))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64) / side
        return np.column_stack([g, np.round(64 * 0.3 * np.sin(3 * g[:, 0]) * np.cos(2 * g[:, 1])) / 64])
    return np.vstack([rng.normal(-0.5, 0.02, (n // 2, 3)), rng.normal(0.5, 0.02, (n - n // 2, 3))])   # clusters


@pytest.mark.parametrize("kind", ["blob", "plane", "lattice", "clusters"])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_normals_over_scale_and_offset(eng, kind, scale, offset):
    """each kind at scale 1e-3 / 1 / 1e3 and at the origin / 1e3 extents away from it"""
    rng = np.random.default_rng(31)
    n = 2500
    pts = np.ascontiguousarray((_cloud(rng, n, kind) + offset * np.array([0.6, -0.48, 0.64])) * scale)
    eng.set_frames([pts], None)
    for k in (10, 16):
        nrm, knn = eng.recompute_normals(0, k, want_knn=True)
        normcheck.check(pts, knn, nrm, "%s scale=%g offset=%g k=%d" % (kind, scale, offset, k))


@pytest.mark.parametrize("z", [0.0, 0.25, 0.1, -3.3, 1000.1])
def test_exactly_planar_cloud_gives_exactly_minus_z(eng, z):
    """constant z: the z row and column of the covariance are exactly zero, the Jacobi rotations never touch them, and the normal is
    EXACTLY (0, 0, -1) — also where k z is not a representable sum, so that a mean accumulated from the raw coordinates would miss z"""
    rng = np.random.default_rng(5)
    pts = np.column_stack([rng.uniform(-0.2, 0.2, 1500), rng.uniform(-0.2, 0.2, 1500), np.full(1500, z)])
    eng.set_frames([pts], None)
    for k in (3, 10, 16):
        nrm = eng.recompute_normals(0, k)
        assert np.all(nrm == np.array([0.0, 0.0, -1.0])), (z, k, np.abs(nrm - [0, 0, -1]).max())


def test_degenerate_neighbourhoods_collinear_and_duplicates(eng):
    """exactly collinear points (a dyadic direction: every coordinate exact) and neighbourhoods of k copies of one point (C = 0): a finite
    unit vector with n_z <= 0, and the Rayleigh criterion still holds (lambda_0 = lambda_1 = 0: any vector across the line passes, one
    along it does not)"""
    rng = np.random.default_rng(6)
    s = np.sort(rng.choice(4096, 700, replace=False)).astype(np.float64)
    line = np.outer(s, [0.25, -0.125, 0.5]) / 64 + [1.0, 2.0, -0.5]
    eng.set_frames([np.ascontiguousarray(line)], None)
    nrm, knn = eng.recompute_normals(0, 10, want_knn=True)
    normcheck.check(line, knn, nrm, "collinear")
    d = np.array([0.25, -0.125, 0.5]); d /= np.linalg.norm(d)
    assert np.abs(nrm @ d).max() <= 1e-12          # across the line
    sites = rng.normal(0, 0.1, (40, 3))
    dup = np.ascontiguousarray(np.repeat(sites, 20, axis=0)[rng.permutation(800)])
    eng.set_frames([dup], None)
    nrm, knn = eng.recompute_normals(0, 10, want_knn=True)
    assert np.all(dup[knn] == dup[:, None, :])      # every neighbourhood is ten copies of its point
    normcheck.check(dup, knn, nrm, "all-duplicate neighbourhoods")


CLEAN = (-1, -3)   # MVICP_ERR_ARG, MVICP_ERR_STATE (include/mvicp.h); -2 is MVICP_ERR_HIP


def _status(ex):
    """the status code of an MvicpError ("mvicp status <code>: <message>")"""
    return int(str(ex).split()[2].rstrip(":"))


@pytest.mark.parametrize("n", [0, 1, 2, 3, 9])
def test_clouds_smaller_than_k_give_a_clean_status_and_leave_the_context_usable(n):
    """n in {0, 1, 2, 3, k - 1} points with k = 10: a clean error status (MVICP_ERR_STATE or MVICP_ERR_ARG, never MVICP_ERR_HIP, no NaN); n = 3 with k = 3 is a legal call
    and gives one finite normal per point.  The same context then computes a regular cloud's normals."""
    rng = np.random.default_rng(8)
    eng = mvicp.Engine(0)
    try:
        small = np.ascontiguousarray(rng.normal(0, 0.1, (n, 3)))
        uploaded = True
        if n == 0:       # an empty cloud may already be refused at upload: equally a clean status
            try:
                eng.set_frames([small], None)
            except MvicpError as ex:
                assert _status(ex) in CLEAN, str(ex)
                uploaded = False
        else:
            eng.set_frames([small], None)
        if uploaded:
            with pytest.raises(MvicpError) as ei:
                eng.recompute_normals(0, 10)
            assert _status(ei.value) in CLEAN, str(ei.value)
        if n == 3:
            nrm, knn = eng.recompute_normals(0, 3, want_knn=True)
            assert np.array_equal(np.sort(knn, axis=1), np.tile(np.arange(3), (3, 1)))
            normcheck.check(small, knn, nrm, "three points, k = 3")
        pts = np.ascontiguousarray(rng.normal(0, 0.1, (500, 3)))
        eng.set_frames([pts], None)
        nrm, knn = eng.recompute_normals(0, 10, want_knn=True)
        normcheck.check(pts, knn, nrm, "after n = %d" % n)
    finally:
        eng.close()
