"""The clouds of the tests of mvicp_fit_normals (tests/test_jet_cpu.py, tests/test_gpu_fit_normals.py)."""
import numpy as np

import knnref
import normcases

VIEWPOINT = (0.1, -0.2, 3.0)


def blob(n=300, seed=3):
    return np.ascontiguousarray(np.random.default_rng(seed).normal(0.0, 0.25, (n, 3)))


def exact_cases():
    """name -> (points, max_nn, radius, viewpoint, degree): the byte-for-byte cases both the scalar loop and the GPU are held to"""
    b = blob()
    dup, line, lat = normcases.duplicates(8, 8), normcases.collinear(60), knnref.shuffled_lattice()
    return {
        "blob-10-2": (b, 10, 0.0, VIEWPOINT, 2),
        "blob-16-3": (b, 16, 0.0, VIEWPOINT, 3),
        "blob-64-3": (b, 64, 0.0, VIEWPOINT, 3),
        "lattice-10-2": (lat, 10, 0.0, None, 2),      # exact ties and exactly singular neighbourhoods: pivots fail
        "lattice-16-3": (lat, 16, 0.0, None, 3),
        "duplicates": (dup, 12, 0.0, (0.0, 0.0, 1.0), 3),   # every neighbourhood is copies of its point: h == 0
        "collinear": (line, 12, 0.0, (1.0, 2.0, 5.0), 2),
        "hybrid-2": (b, 12, 0.17, (0.0, 0.0, 2.0), 2),      # rows from empty to full: some c_i < M
        "hybrid-3": (b, 16, 0.2, (0.0, 0.0, 2.0), 3),
    }


def plane(seed, n=600):
    """a plane in general position: an orthonormal (u, v, nrm) from random vectors, points o + s u + t v -> (points, nrm)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    st = rng.uniform(-1.0, 1.0, (n, 2))
    return np.ascontiguousarray(rng.normal(size=3) + st @ q[:, :2].T), q[:, 2]


PARABOLOID_HALF_WIDTH = 1e-4


def paraboloid(seed=11, n=2000, half_width=PARABOLOID_HALF_WIDTH):
    """z = 0.3 x^2 - 0.2 x y + 0.1 y^2 + 0.05 x over the square |x|, |y| <= half_width, sampled uniformly at random -> (points, analytic unit
    normals).  Why the window is small: the height of this surface over a plane that is TILTED against the z axis (every tangent plane off
    the apex, and every PCA plane) is the root of a quadratic, a polynomial in (X, Y) only up to terms of relative size (kappa r)^2, where
    kappa <= 0.69 is the largest principal curvature and r the radius of a neighbourhood.  A normal exact to 1e-9 rad can therefore be asked
    for only where (kappa r)^2 is well below 1e-9: r <= 2e-5 gives 2e-10.  2000 points over a window of half-width 1e-4 have their 16
    nearest within r ~ 1e-5 (2e-5 at the rim).  A PCA normal errs in first order, kappa r times the unevenness of the sample, 1e-6 here."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-half_width, half_width, (2, n))
    z = 0.3 * x * x - 0.2 * x * y + 0.1 * y * y + 0.05 * x
    g = np.stack([-(0.6 * x - 0.2 * y + 0.05), -(-0.2 * x + 0.2 * y), np.ones(n)], 1)
    return np.ascontiguousarray(np.stack([x, y, z], 1)), g / np.linalg.norm(g, axis=1)[:, None]
