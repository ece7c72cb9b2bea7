"""Problems placed away from the origin, and the query map restated in numpy.  Test infrastructure only.

`place` moves a registration problem (pts, nor, poses, cutoff) somewhere else; the placed problem is always compared with the oracle
on the PLACED inputs, never with the unplaced run.  A scripted pose sequence is generated on the unit problem (`scripted_poses`,
moves applied as pose @ T_small like the cache tests of test_gpu_parity.py) and every pose set of it is placed, so that the physical
motion of a round is the same under every placement.

`query_block`, `xf_point` and `inverse3` restate csrc/search_plan.h:fill_query_xf / inverse3 and csrc/nn_metric.h:xf_point operation by
operation; run on np.longdouble inputs the same code is the extended-precision map."""
import numpy as np

from mvicp import synth

LD = np.longdouble

WL = np.array([-50.0, -700.0, -470.0])          # a local site frame
W1E6 = np.array([1e6, -7e5, 3e5])
WU = np.array([5e5, 4.1e6, 300.0])              # UTM easting / northing / height
DU3 = np.array([12.5, -3.25, 7.75])             # frames k = 1 mod 3: a scan from another station, WU3 = WU + DU3

# name -> (scale s of the data, shift W of the points, world shift of the poses, what the frames k = 1 mod 3 do with DU3)
#   "moved":  the station's own origin is elsewhere: its points are shifted by -c_k, c_k = R_k^T DU3 at the initial pose, and every pose
#             of it gets + R c_k — at the initial poses exactly "translation + WU3", and the scene stays where it is in every round.  The
#             relative translation v = Rd^-1 (ts - td) of its edges is ~15 m and its queries still have neighbours.
#   "apart":  translation + DU3 only, points untouched: the scan itself ends up 15 m away and every query of its edges is without a
#             neighbour (exactness of that path only: no cache can answer a moving query that has no neighbour).
PLACEMENTS = {
    "unit": (1.0, None, None, None),
    "local": (1.0, WL, None, None),
    "mm_local": (1e-3, WL, None, None),
    "local1e6": (1.0, W1E6, None, None),
    "utm": (1.0, None, WU, "moved"),
    "mm_utm": (1e-3, WL, WU, "moved"),
    "utm_apart": (1.0, None, WU, "apart"),
}


def place_scale(name):
    return PLACEMENTS[name][0]


def place_points(name, p, shift_extra=None):
    """The point map of a placement, p' = s p + W (what nn_query sees: it takes no pose)."""
    s, shift, _, _ = PLACEMENTS[name]
    p = np.asarray(p, dtype=np.float64)
    if s != 1.0:
        p = p * s
    if shift is not None:
        p = p + shift
    if shift_extra is not None:
        p = p + shift_extra
    return np.ascontiguousarray(p)


class Placement:
    """One placement of one problem: fixed by the name and the problem's INITIAL poses (the station offsets c_k are taken there).
    Points p' = s p + W_k keep their world position, scaled by s, under t' = s t - R W_k; the world shift is added on top."""

    def __init__(self, name, init_poses):
        self.name = name
        self.s, shift, self.world, self.du3 = PLACEMENTS[name]
        init_poses = np.asarray(init_poses, dtype=np.float64)
        base = np.zeros(3) if shift is None else shift
        self.shift = []
        for k, P in enumerate(init_poses):
            moved = self.du3 == "moved" and k % 3 == 1
            self.shift.append(base - DU3 @ P[:3, :3] if moved else base)        # c_k = R^T DU3, as a row: DU3^T R

    def points(self, k, p):
        return np.ascontiguousarray(np.asarray(p, dtype=np.float64) * self.s + self.shift[k])

    def poses(self, poses):
        out = []
        for k, P in enumerate(np.asarray(poses, dtype=np.float64)):
            S = P.copy()
            S[:3, 3] = self.s * S[:3, 3] - S[:3, :3] @ self.shift[k]
            if self.world is not None:
                S[:3, 3] = S[:3, 3] + self.world
                if self.du3 == "apart" and k % 3 == 1:
                    S[:3, 3] = S[:3, 3] + DU3
            out.append(S)
        return np.array(out)

    def cutoff(self, c):
        c = np.float32(c)
        return c if self.s == 1.0 else np.float32(c * np.float32(self.s))


def place(name, pts, nor, poses, cutoff):
    """-> (pts', nor, poses', cutoff', the Placement) of the placed problem; `poses` are the problem's initial poses, later pose sets go
    through Placement.poses.  Normals are invariant (shifts and a uniform scale)."""
    pl = Placement(name, poses)
    return [pl.points(k, p) for k, p in enumerate(pts)], nor, pl.poses(poses), pl.cutoff(cutoff), pl


def small_motion(rng, mag):
    T = np.eye(4)
    T[:3, :3] = synth.so3_exp(rng.normal(0, mag / 0.4, 3))
    T[:3, 3] = rng.normal(0, mag, 3)
    return T


def exact_step(rng, mag, direction):
    """A rigid motion of exactly the given size: a translation of length mag along `direction` (a unit vector in the moved frame's own
    coordinates), a rotation of mag / 0.4 about a random axis.  (small_motion draws both from a normal distribution: a single draw is
    anything from 0.3 to 3 times its nominal size, along any direction.)"""
    v = rng.normal(0, 1, 3)
    T = np.eye(4)
    T[:3, :3] = synth.so3_exp(v / np.linalg.norm(v) * (mag / 0.4))
    T[:3, 3] = np.asarray(direction, dtype=np.float64) * mag
    return T


def scripted_poses(init, mags, seed):
    """[init, init moved by mags[0], that moved by mags[1], ..., the last once more]: frame 0 stays, frame k >= 1 gets pose @ T_small."""
    rng = np.random.default_rng(seed)
    seq = [np.array(init, dtype=np.float64)]
    for mag in mags:
        P = seq[-1].copy()
        for k in range(1, len(P)):
            P[k] = P[k] @ small_motion(rng, mag)
        seq.append(P)
    seq.append(seq[-1].copy())
    return seq


# ---------------------------------------------------------------- the query map, operation by operation
def inverse3(m):
    """csrc/api.cpp:inverse3 (Eigen's cofactor inverse) in the dtype of m."""
    def cof(i, j):
        return m[(i + 1) % 3, (j + 1) % 3] * m[(i + 2) % 3, (j + 2) % 3] - m[(i + 1) % 3, (j + 2) % 3] * m[(i + 2) % 3, (j + 1) % 3]
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = (c00 * m[0, 0] + c10 * m[1, 0]) + c20 * m[2, 0]
    invdet = 1 / det
    r = np.empty((3, 3), dtype=m.dtype)
    r[0, 0] = c00 * invdet; r[0, 1] = c10 * invdet; r[0, 2] = c20 * invdet
    r[1, 0] = cof(0, 1) * invdet; r[1, 1] = cof(1, 1) * invdet; r[1, 2] = cof(2, 1) * invdet
    r[2, 0] = cof(0, 2) * invdet; r[2, 1] = cof(1, 2) * invdet; r[2, 2] = cof(2, 2) * invdet
    return r


def query_block(Ps, Pd):
    """fill_query_xf: (Rs, ts, Rd^-1, td) of a directed pair, in float64 (Rd^-1 by the fp64 cofactor inverse, as stored)."""
    Ps = np.asarray(Ps, dtype=np.float64); Pd = np.asarray(Pd, dtype=np.float64)
    return Ps[:3, :3].copy(), Ps[:3, 3].copy(), inverse3(Pd[:3, :3].copy()), Pd[:3, 3].copy()


def xf_point(block, p, dtype=np.float64):
    """nn_metric.h:xf_point on the rows of p: g = ((R0 p0 + R1 p1) + R2 p2) + ts; u = g - td; q = (Ri0 u0 + Ri1 u1) + Ri2 u2, every
    operation rounded on its own in `dtype` (numpy never contracts).  dtype = LD: the same stored block, evaluated in extended precision."""
    R, ts, Ri, td = (np.asarray(a).astype(dtype) for a in block)
    p = np.asarray(p).astype(dtype)
    g = ((R[:, 0] * p[:, 0:1] + R[:, 1] * p[:, 1:2]) + R[:, 2] * p[:, 2:3]) + ts
    u = g - td
    return (Ri[:, 0] * u[:, 0:1] + Ri[:, 1] * u[:, 1:2]) + Ri[:, 2] * u[:, 2:3]


def xf_error(block, p):
    """max over the rows of p of |q_fp64 - q_longdouble| (Euclidean)."""
    d = xf_point(block, p).astype(LD) - xf_point(block, p, LD)
    return float(np.sqrt((d * d).sum(1)).max())


def parent_allowance(block, rmax):
    """The allowance before the derived bound, as a literal: 1e-12 (scale (rmax + 1) + 1), scale = max |entry of M = Rd^-1 Rs or of
    v = Rd^-1 (ts - td)|.  Kept for two assertions: the upper limit of the new value, and that the old one fails far from the origin."""
    R, ts, Ri, td = block
    scale = max(np.abs(Ri @ R).max(), np.abs(Ri @ (ts - td)).max())
    return 1e-12 * (scale * (rmax + 1.0) + 1.0)


def random_rotation(rng):
    return synth.so3_exp(rng.normal(0, 1, 3))


def pose(R, t):
    P = np.eye(4)
    P[:3, :3] = R; P[:3, 3] = t
    return P


# ---------------------------------------------------------------- queries on bisector planes
BISECTOR_H = 2.0 ** -10
BISECTOR_SIDE = 32


def bisector_problem(T, seed, n=20000):
    """Two frames with a common world translation T (1, -0.7, 0.3) + N(0, 0.05).  Frame 0 (target): a 32 x 32 lattice of spacing 2^-10 at
    z = 0.  Frame 1 (source): n points computed in extended precision so that their images under the stored query transform lie within
    +-3e-10 of the bisector plane between two x-neighbours of the lattice, 0.1 .. 0.4 spacings above it: best and second-best distance
    differ by less than a nanometre, so a displacement bound that is wrong by 1e-10 decides which target a cache hit keeps.
    -> (pts [target, source], poses (2, 4, 4), the wanted images (n, 3))"""
    rng = np.random.default_rng(seed)
    h, side = BISECTOR_H, BISECTOR_SIDE
    g = np.arange(side) * h
    tgt = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    tgt = np.ascontiguousarray(np.column_stack([tgt, np.zeros(len(tgt))]))
    W = T * np.array([1.0, -0.7, 0.3])
    Ps = pose(random_rotation(rng), W + rng.normal(0, 0.05, 3))
    Pd = pose(random_rotation(rng), W + rng.normal(0, 0.05, 3))
    ix = rng.integers(0, side - 1, n); iy = rng.integers(0, side, n)
    qd = np.column_stack([(ix + 0.5) * h + rng.uniform(-3e-10, 3e-10, n), iy * h + rng.uniform(-0.2, 0.2, n) * h, rng.uniform(0.1, 0.4, n) * h])
    R, ts, Ri, td = query_block(Ps, Pd)
    # q = Ri (R p + ts - td)  <=>  p = R^-1 (Ri^-1 q - (ts - td)), in extended precision from the stored fp64 block
    u = qd.astype(LD) @ inverse3(Ri.astype(LD)).T - (ts.astype(LD) - td.astype(LD))
    p = np.ascontiguousarray((u @ inverse3(R.astype(LD)).T).astype(np.float64))
    return [tgt, p], np.array([Pd, Ps]), qd


def brute_two_nearest(q, tgt, chunk=2048):
    """(index of the nearest, best d2, second d2) in the reference's operation order (nn_metric.h:dist2), first index on ties."""
    idx, best, second = [], [], []
    for a in range(0, len(q), chunk):
        d = q[a:a + chunk, None, :] - tgt[None]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = np.argmin(d2, axis=1)
        r = np.arange(len(i))
        idx.append(i); best.append(d2[r, i].copy())
        d2[r, i] = np.inf
        second.append(d2.min(axis=1))
    return np.concatenate(idx), np.concatenate(best), np.concatenate(second)
