"""mvicp_recompute_normals on the ways out of the growing-block traversal (csrc/knn_traverse.h) that its kernel shares with the other
neighbourhood kernels: a block that stops at once, one that grows first, one that exceeds 2 n cells (the cloud itself is scanned) and one
that covers the grid.  Which way a point takes is derived from the grid the library built (tests/traverseref.py) and from nanoflann's
distances alone; the lists then equal nanoflann's element for element and the normals pass tests/normcheck.py.

A block that covers the grid has as many cells as the grid, and it is scanned only if those are at most 2 n; no block of such a grid
exceeds 2 n cells.  So no cloud of more than 13 points has both a "cloud" and a "grid" point, and the two ways are asserted on two
clouds: "far" reaches the first three, "corner" (25 points of the same lattice) the fourth."""
import numpy as np
import pytest

import mvicp
import normcheck
import traverseref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = mvicp.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def reference(refnn):
    """nanoflann's lists of k (what the kernel must return) and of k + 1 (the ties at the k-th place) for both clouds and both k, once"""
    if refnn is None:
        return None
    return {(kind, k): refnn.knn_self(traverseref.patch_cloud(kind), k) + refnn.knn_self(traverseref.patch_cloud(kind), k + 1)
            for kind in ("far", "corner") for k in (10, 16)}


@pytest.mark.parametrize("k", [10, 16])
@pytest.mark.parametrize("kind", ["far", "corner"])
def test_recompute_normals_on_every_way_out(eng, reference, kind, k):
    if reference is None:
        pytest.skip("oracle/_ref was not built")
    pts = traverseref.patch_cloud(kind)
    n = len(pts)
    gi, gd, _, gd1 = reference[(kind, k)]
    assert np.array_equal(gd, gd1[:, :k])
    eng.set_frames([pts], None)
    sc = eng.get_structure(0, "scalars")
    # the kernel stops once its k-th distance (the point itself at place 0) lies inside the block's faces; it walks no box tree
    ways, radii, _ = traverseref.exits(pts, sc, n, np.sqrt(gd[:, k - 1]), tree=False)
    ways = np.array(ways)
    stop1, stop2 = (ways == "stop") & (radii == 1), (ways == "stop") & (radii >= 2)
    ties = int((stop2 & (gd1[:, k - 1] == gd1[:, k])).sum())
    print(kind, "k", k, "cell", sc[6], "dims", sc[:3], {w: int((ways == w).sum()) for w in np.unique(ways)}, "stop at r = 1:", int(stop1.sum()),
          "at r >= 2:", int(stop2.sum()), "of those tied at the k-th place:", ties)
    if kind == "far":
        assert n == 416 and stop1.sum() >= 1 and stop2.sum() >= 1 and (ways == "cloud").sum() >= 1
        assert ties >= 20
    else:
        assert (ways == "grid").sum() >= 1 and stop2.sum() >= 1
    nrm, knn = eng.recompute_normals(0, k, want_knn=True)
    e = pts[:, None, :] - pts[knn]
    myd = (e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1]) + e[:, :, 2] * e[:, :, 2]
    assert np.array_equal(myd, gd), (kind, k)
    assert np.array_equal(knn, gi), (kind, k, int((~np.all(knn == gi, axis=1)).sum()))
    normcheck.check(pts, knn, nrm, "patch cloud %s, k = %d" % (kind, k))
