"""Generates tests/golden/deep_tie_nn.npz: what the REAL vendored nanoflann (oracle/_ref/libref_nanoflann.so, built by oracle/Makefile from
the reference's include/nanoflann.hpp) answers, 1-NN index and squared distance, on the clouds of tests/test_tie_walk_cpu.py — so that
that test and tests/test_gpu_deep_tie.py run where oracle/_ref cannot be built.  The inputs are regenerated from their recipes by the
tests themselves; only the outputs are stored.

Run where oracle/_ref is built:   python tests/golden/make_deep_tie_nn.py

deep_tie_nn.npz
  n{200,300,900}_self_idx, _self_d2    : findNeighbors(1) of every point of deep_cloud(n) against the cloud itself (every d2 = 0)
  n{200,300,900}_aside_idx, _aside_d2  : the same for deep_queries(cloud)[1] (the points moved aside along y)
  lattice_self_idx, lattice_self_d2    : the same for test_knn_tie_order.lattice_points() against itself
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "mv-lm-icp_amd"))
import orclib  # noqa: E402
import test_knn_tie_order as K  # noqa: E402
import test_tie_walk_cpu as T  # noqa: E402


def main():
    ref = orclib.load_ref()
    assert ref is not None, "oracle/_ref not built (needs the reference's nanoflann.hpp)"
    out = {}
    for n in T.DEEP_N:
        pts = T.deep_cloud(n)
        for tag, q in zip(("self", "aside"), T.deep_queries(pts)):
            i, d = ref.query(pts, q)
            out[f"n{n}_{tag}_idx"] = i.astype(np.int32)
            out[f"n{n}_{tag}_d2"] = d.astype(np.float64)
    lat = K.lattice_points()
    i, d = ref.query(lat, lat)
    out["lattice_self_idx"] = i.astype(np.int32); out["lattice_self_d2"] = d.astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "deep_tie_nn.npz"), **out)
    print("wrote deep_tie_nn.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
