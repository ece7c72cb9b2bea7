"""The ways out of the growing-block traversal (csrc/knn_traverse.h) in numpy, from the scalars of the grid the library built
(Engine.get_structure(frame, "scalars")): which way every point of a cloud takes, at which block radius, and how near a face of the grid
that the stop rule leaves out was.  The tests of the traversal's users assert from it that a cloud reaches the ways it is meant to."""
import numpy as np


def exits(p, sc, n, dist, tree=True):
    """-> (ways, radii, left_out), one entry per point of p.  dist: the distance at which a point's search may stop, one number for all
    points (a radius search) or one per point (a k-nearest search: the reference's k-th distance, the point itself counted as the kernel
    counts it).
    ways: "stop" (the block holds dist), "grid" (the block covers the grid), "cloud" (the block exceeds 2 n cells: the cloud is scanned)
    or "tree" (the block of radius 4 has not finished: the box tree; without a tree that way does not exist and the block keeps
    growing).  The face distances are taken with a margin of a hundredth of a cell, so a point this function calls "stop", "cloud" or
    "tree" takes that way whatever the rounding of the kernel's own face arithmetic (its factor 0.999 on the face distance stays inside
    the margin while the block's radius is below 9); a point inside the margin is an "edge".
    radii: the radius of the last block.
    left_out: the smallest distance to the plane of a face of that block which lies at or beyond the grid's boundary and therefore does
    not enter the stop rule (+inf: no such face)."""
    dims, o, h = sc[:3].astype(np.int64), sc[3:6], float(sc[6])
    dist = np.broadcast_to(np.asarray(dist, dtype=np.float64), (len(p),))
    ways, radii, left_out = [], [], []
    for q, d in zip(p, dist):
        c = np.clip(np.floor((q - o) / h), 0, dims - 1).astype(np.int64)
        r = 1
        while True:
            lo, hi = np.maximum(c - r, 0), np.minimum(c + r, dims - 1)
            low = [(q[a] - (o[a] + (c[a] - r) * h), c[a] - r > 0) for a in range(3)]
            high = [(o[a] + (c[a] + r + 1) * h - q[a], c[a] + r < dims[a] - 1) for a in range(3)]
            m = [v for v, inner in low + high if inner]
            skipped = min([v for v, inner in low + high if not inner], default=np.inf)
            if r > 1 and int(np.prod(hi - lo + 1)) > 2 * n:
                way = "cloud"
            elif not m:
                way = "grid"
            elif d <= min(m) - 0.01 * h:
                way = "stop"
            elif d <= min(m) + 0.01 * h:
                way = "edge"
            elif r == 4 and tree:
                way = "tree"
            else:
                r += 1
                continue
            ways.append(way); radii.append(r); left_out.append(skipped)
            break
    return ways, np.array(radii), np.array(left_out)


def patch_cloud(kind):
    """A planar lattice patch like a range image (pitch 0.01, z quantised to the pitch: exact ties).
    "far": 14 x 20 points, beside them 10 x 12 points at four times the pitch, so that the 3^3 cells around a point of the sparse half
    hold fewer than 16 points; a cluster of 8 points 0.4 above the patch, whose growing block passes 2 n cells before it holds 10
    points; and the eight corners of a box around everything, so that no block is cut short by a face of the grid.  416 points.
    "corner": 5 x 5 points of the sparse half alone, a grid of 32 cells that the blocks of its outer points cover.
    Both shuffled."""
    rng = np.random.Generator(np.random.PCG64(77))
    dense = [[x, y] for x in range(14) for y in range(20)]
    sparse = [[16 + 4 * x, 4 * y] for x in range(10) for y in range(12)]
    xy = np.array(dense + sparse if kind == "far" else [[16 + 4 * x, 4 * y] for x in range(5) for y in range(5)], dtype=np.float64)
    parts = [np.column_stack([xy, np.round(0.8 * np.sin(0.11 * xy[:, 0]) * np.cos(0.07 * xy[:, 1]))])]
    if kind == "far":
        parts.append(np.array([23.0, 18.0, 40.0]) + rng.uniform(-0.4, 0.4, size=(8, 3)))
        parts.append(np.array([[x, y, z] for x in (-30.0, 80.0) for y in (-30.0, 80.0) for z in (-30.0, 80.0)]))
    p = np.concatenate(parts, 0) * 0.01
    return np.ascontiguousarray(p[rng.permutation(len(p))])
