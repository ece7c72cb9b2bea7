"""The clouds of the tests of mvicp_smooth_points (tests/test_smooth_cpu.py, tests/test_gpu_smooth*.py): the bump surface of matchref with
noise along its analytic normals, the distance of a point to that surface, and a sphere."""
import functools

import numpy as np

import initref
import matchref
import smoothref
from test_normals_cpu import VIEW

SMOOTH_NN, SMOOTH_DEGREE = 30, 2      # the smoothing of the registration cases
FIT_NN, FIT_DEGREE = 16, 3            # the normals they register on


def height(xy):
    """the bump field of matchref.bumps at the (m, 2) positions xy -> (z (m,), gradient (m, 2))"""
    c, a, s = matchref._bump_field()
    dx, dy = xy[:, 0, None] - c[None, :, 0], xy[:, 1, None] - c[None, :, 1]
    g = a[None, :] * np.exp(-(dx * dx + dy * dy) / (2.0 * s[None, :] ** 2))
    return g.sum(1), np.stack([(g * (-dx / s[None, :] ** 2)).sum(1), (g * (-dy / s[None, :] ** 2)).sum(1)], 1)


def surface_distance(p, steps=6):
    """the distance of every row of p to the bump surface: the foot point is found by moving it, `steps` times, to where the normal line
    through it passes closest to p.  At the noise levels of the tests (well below the radii of curvature) the iteration converges to
    rounding in three steps."""
    q = p[:, :2].copy()
    for _ in range(steps):
        z, g = height(q)
        m = np.concatenate([-g, np.ones((len(p), 1))], 1)
        m /= np.linalg.norm(m, axis=1, keepdims=True)
        s = np.concatenate([q, z[:, None]], 1)
        d = ((p - s) * m).sum(1)
        q = (p - d[:, None] * m)[:, :2]
    z, _ = height(q)
    return np.linalg.norm(p - np.concatenate([q, z[:, None]], 1), axis=1)


def rms(x):
    return float(np.sqrt((x * x).mean()))


@functools.lru_cache(maxsize=None)
def noisy_bumps(sigma):
    """matchref.bumps(1500, 100) with N(0, (sigma spacings)^2) added along the analytic normal from PCG64(7) -> (points, spacing)"""
    p, nrm = matchref.bumps(1500, 100)
    spacing = matchref.e2e_clouds(False)["spacing"]
    if sigma == 0:
        return p, spacing
    return smoothref.noisy(p, nrm, sigma * spacing, np.random.Generator(np.random.PCG64(7))), spacing


@functools.lru_cache(maxsize=None)
def noisy_pair(partial, sigma=0.5):
    """matchref.e2e_clouds(partial) with both clouds noised along their analytic normals: one PCG64(9) generator, src drawn first, then dst.
    -> the dict of e2e_clouds with the noisy src / dst, the clean ones under clean_src / clean_dst and the two viewpoints of
    test_jet_cpu.with_normals under view_src / view_dst"""
    cl = dict(matchref.e2e_clouds(partial))
    rng = np.random.Generator(np.random.PCG64(9))
    cl["clean_src"], cl["clean_dst"] = cl["src"], cl["dst"]
    cl["src"] = smoothref.noisy(cl["src"], cl["src_nrm"], sigma * cl["spacing"], rng)
    cl["dst"] = smoothref.noisy(cl["dst"], cl["dst_nrm"], sigma * cl["spacing"], rng)
    cl["view_src"], cl["view_dst"] = VIEW, cl["truth"][:3, :3] @ VIEW + cl["truth"][:3, 3]
    return cl


@functools.lru_cache(maxsize=None)
def noisy_fixture(sigma=0.5):
    """initref.fixture_clouds() with every view noised along its analytic normals by sigma spacings, one PCG64(9) generator, view 0 first"""
    fx = dict(initref.fixture_clouds())
    rng = np.random.Generator(np.random.PCG64(9))
    fx["xyz"] = [smoothref.noisy(p, nn, sigma * fx["spacing"], rng) for p, nn in zip(fx["xyz"], fx["nrm"])]
    return fx


def sphere(rings=10, spacing=0.1, R=2.0, centre=(0.3, -0.2, 0.5)):
    """A cap of the sphere of radius R about `centre`: the hexagonal lattice of `rings` rings (10: 331 points) and the given spacing in the
    plane z = 0, lifted to the sphere about its +z pole.  Why the spacing is small against R: over a neighbourhood of radius r the height
    of a sphere above its tangent plane is r^2 / 2R (1 + r^2 / 4R^2 + ...), so a quadratic fit overstates the curvature by about
    r^2 / 4R^2.  16 neighbours of this lattice lie within r ~ 0.21 (0.35 at the rim): 0.3 % (0.8 %), well inside the 3 % the test allows."""
    ij = np.array([(i, j) for i in range(-rings, rings + 1) for j in range(-rings, rings + 1) if abs(i + j) <= rings], dtype=np.float64)
    x, y = spacing * (ij[:, 0] + 0.5 * ij[:, 1]), spacing * (0.75 ** 0.5) * ij[:, 1]
    return np.ascontiguousarray(np.asarray(centre) + np.stack([x, y, np.sqrt(R * R - x * x - y * y)], 1))
