"""Generates tests/golden/nanoflann_synthetic.npz: what the REAL vendored nanoflann (oracle/_ref/libref_nanoflann.so, built by
oracle/Makefile from the reference's include/nanoflann.hpp) answers on the seeded synthetic clouds of tests/test_knn_tie_order.py and
tests/test_oracle_nn.py, so that those tests run where oracle/_ref cannot be built.  The inputs are regenerated from their seeds by
the tests themselves; only the outputs are stored.

Run where oracle/_ref is built:   python tests/golden/make_synthetic_nn.py

nanoflann_synthetic.npz
  lattice_knn_idx     : knnSearch(k = 10) around every point of test_knn_tie_order.lattice_points() (4000 points on 21^3 sites), nanoflann's order
  degenerate_knn_idx  : the same on test_knn_tie_order.degenerate_points() (geometric progression + duplicates: a 900-level tree)
  query_idx, query_d2 : 1-NN index / squared distance of test_oracle_nn.synthetic_queries() q  against its dst
  query_far_idx, _d2  : the same for q2 (queries exactly on points and far outside the cloud)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.join(os.path.dirname(TESTS), "mv-lm-icp_amd"))
import orclib  # noqa: E402
import test_knn_tie_order as T  # noqa: E402
import test_oracle_nn as O  # noqa: E402


def main():
    ref = orclib.load_ref()
    assert ref is not None, "oracle/_ref not built (needs the reference's nanoflann.hpp)"
    out = {}
    for name, pts in (("lattice_knn_idx", T.lattice_points()), ("degenerate_knn_idx", T.degenerate_points())):
        out[name] = ref.knn_self(pts, 10)[0].astype(np.int32)
    dst, q, q2 = O.synthetic_queries()
    for name, qq in (("query", q), ("query_far", q2)):
        i, d = ref.query(dst, qq)
        out[name + "_idx"] = i.astype(np.int32)
        out[name + "_d2"] = d.astype(np.float64)
    np.savez_compressed(os.path.join(HERE, "nanoflann_synthetic.npz"), **out)
    print("wrote nanoflann_synthetic.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
