"""Python-side harness for libmvicp_hip.so (tests / bench only — the product is the C-ABI library).

`lib`   : ctypes binding of include/mvicp.h (one class, `Engine`, mirroring the call order of the
          reference's main_multiview.cpp loop).
`synth` : the build-owned deterministic synthetic multi-view generator.
`io`    : the reference's on-disk formats (.xyz clouds, 4x4 row-major pose text).
"""
from . import lib, synth, io  # noqa: F401
from .lib import Engine, MvicpError, load_library, graph_from_overlap, overlap_sample_indices, outlier_threshold, cluster_keep_rule, plane_from_moments, reject_by_mask, cache_allowance, match_pairs, coarse_align, poses_from_pairs, init_from_clouds, signs_from_agreement, orient_frames, principal_curvatures  # noqa: F401
