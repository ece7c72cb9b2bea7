"""The Frame-mirror harness (mv-lm-icp_amd/bin/frame_harness.so, tests/frame_harness.cpp) exists after the build, exports what
tests/framelib.py binds, and hands the mirror's exceptions over as a status plus the message -- all without a GPU."""
import os
import re

import numpy as np
import pytest

import framelib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def defined_symbols():
    txt = open(os.path.join(ROOT, "tests", "frame_harness.cpp")).read()
    txt = txt[txt.index('extern "C" {'):]
    return sorted(set(re.findall(r"^(?:const char\*|int) (fh_[a-z0-9_]+)\(", txt, flags=re.M)))


def test_harness_exports_what_the_wrapper_binds():
    assert os.path.exists(framelib.HARNESS_PATH), "the build did not produce bin/frame_harness.so"
    lib = framelib.load()
    syms = defined_symbols()
    assert len(syms) >= 40
    for s in syms:
        assert hasattr(lib, s), f"{s} defined in tests/frame_harness.cpp but not exported"
    assert sorted(framelib.SYMBOLS) == syms, "tests/framelib.py out of sync with tests/frame_harness.cpp"


def test_exceptions_cross_the_boundary_as_status_and_text():
    m = framelib.Mirror()
    m.reset_all()
    try:
        with pytest.raises(framelib.MirrorError, match="frame_harness: no such slot"):
            m.get_pose(3)
        s = m.slot_create()
        with pytest.raises(framelib.MirrorError, match=r"mvicp: getClosestPoint on an empty cloud"):
            m.get_closest_point(s, [0.0, 0.0, 0.0])
        cloud = np.arange(36, dtype=np.float64).reshape(12, 3)
        m.set_pts(s, cloud)
        assert np.array_equal(m.get_pts(s), cloud) and len(m.get_nor(s)) == 0
        for k in (2, 17, 13):
            with pytest.raises(framelib.MirrorError, match=r"mvicp: getNeighbours supports 3 <= num_results <= 16 \(and <= the cloud's size\)"):
                m.get_neighbour_indices(s, k, 12)
        # same storage: the Frame constructed after the destroyed one lives at its address and starts empty
        addr = m.slot_address(s)
        m.slot_destroy(s)
        with pytest.raises(framelib.MirrorError, match="the slot's frame is destroyed"):
            m.get_pts(s)
        m.slot_recreate(s)
        assert m.slot_address(s) == addr and len(m.get_pts(s)) == 0 and m.get_version(s) == 0
        # the spare vector: a swap hands the buffer over and back
        m.set_pts(s, cloud)
        m.stash_set(cloud[:5] + 1.0)
        m.stash_swap_pts(s)
        assert np.array_equal(m.get_pts(s), cloud[:5] + 1.0)
        m.stash_swap_pts(s)
        assert np.array_equal(m.get_pts(s), cloud)
        import torch
        if not torch.cuda.is_available():   # no device: the library's refusal arrives with its message (no CPU fallback)
            m.vec_set(0, [s])
            m.set_neighbours(s, [0])
            with pytest.raises(framelib.MirrorError, match="no CPU fallback"):
                m.closest_to_neighbours(0, 0, 0.05)
            with pytest.raises(framelib.MirrorError, match="no CPU fallback"):
                m.get_closest_point(s, [0.0, 0.0, 0.0])
    finally:
        m.reset_all()
