"""The masked search, stated in numpy (TEST INFRASTRUCTURE; include/mvicp.h "reject masks").

A masked search is the unmasked search with the pairs on flagged points taken out AFTER the nearest neighbour was found: a query whose
neighbour is flagged is dropped, never re-matched.  Counts, lists, stored distances and the weight follow from the kept pairs alone."""
import numpy as np

import mvicp


def masked(first, second, dist, src_mask, dst_mask):
    """(first, second, dist) of the UNMASKED search of an edge, the source's / the target's reject mask (per point, original order, nonzero
    = reject; either may be None) -> (first, second, dist, weight) of the masked search: reject_by_mask over the pairs, their distances,
    and weight = float32(1.5 x the upper median of the kept distances), 0 for an empty list."""
    first = np.ascontiguousarray(first, dtype=np.int32).reshape(-1)
    second = np.ascontiguousarray(second, dtype=np.int32).reshape(-1)
    dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
    if not (len(first) == len(second) == len(dist)):
        raise ValueError("first, second and dist differ in length")
    kf, ks = mvicp.reject_by_mask(first, second, src_mask, dst_mask)
    # reject_by_mask keeps the order, and a search lists every source point at most once: the kept rows are those whose `first` survived
    keep = np.isin(first, kf, assume_unique=True)
    assert kf.tobytes() == first[keep].tobytes() and ks.tobytes() == second[keep].tobytes()
    kd = np.ascontiguousarray(dist[keep])
    weight = np.float32(1.5 * np.sort(kd)[len(kd) // 2]) if len(kd) else np.float32(0)
    return kf, ks, kd, weight
