#!/usr/bin/env python3
"""Times the neighbour search (Engine.knn_search, csrc/knn.hip) and its yardsticks.

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case, first the result on a 5000-point subsample cloud is compared with the numpy statement of the contract (tests/knnref.py).  Then
every configuration gets WARM untimed and REPS timed calls of mvicp_knn_search, each from a drained stream to the call's return (the call
waits for its result; the fetch is not timed): median, min and max in ms, and next to it the library's own profile scopes ("knn_key",
"knn_search", "knn_count", "knn_fill", "knn_order": HIP events on its stream) over further calls:
  self      self mode at k = 8 / 16 / 32 / 64; next to it "outlier_knn" at the same k (k <= 32: the values-only traversal, the floor this
            kernel cannot beat) and the "normals" scope of mvicp_recompute_normals at k = 10 and 16 with knn_out (the only earlier route
            to indexed lists), each on an engine of its own, same cloud, same process
  queries   m = n queries (the cloud under a small rigid motion) and m = 4096 uniform random queries in the bounding box, k = 8, with
            option "knn_order" 1 and 0; and k = 1 next to mvicp_nn_query (its wall time includes its own copies and allocations)
  all       all mode in self mode at the radius whose rows hold about 30 neighbours (the median distance to the 31st candidate over a sample of rows)
One JSON line per measurement.

    python tools/knn_bench.py [--cases one200k,one1m] [--reps 7] [--warm 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvicp  # noqa: E402
import knnref  # noqa: E402
from mvicp import synth  # noqa: E402

SCOPES = ("knn_key", "knn_search", "knn_count", "knn_fill", "knn_order")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}


def report(**kw):
    print(json.dumps(kw), flush=True)


def search_only(eng, q, k, radius):
    m = 0 if q is None else len(q)
    st = eng.lib.mvicp_knn_search(eng.h, 0, None if q is None else q.ctypes.data, m, k, radius)
    if st < 0:
        raise SystemExit(eng.lib.mvicp_last_error().decode())
    return st


def timed(eng, fn, warm, reps):
    ms = []
    for r in range(warm + reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if r >= warm:
            ms.append(1e3 * (t1 - t0))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps}


def measure(eng, what, q, k, radius, args, **kw):
    t = timed(eng, lambda: search_only(eng, q, k, radius), args.warm, args.reps)
    total = search_only(eng, q, k, radius)
    eng.profile(1); eng.profile_reset()
    for _ in range(args.reps):
        search_only(eng, q, k, radius)
    split = {s: eng.profile_get(s)[0] / args.reps for s in SCOPES}
    eng.profile(0)
    report(what=what, k=k, radius=radius, m=(eng.npts[0] if q is None else len(q)), entries=int(total), kernels_ms=sum(split.values()),
           **{s: v for s, v in split.items() if v > 0}, **t, **kw)
    return split


def scope_ms(eng, fn, scope, args):
    for _ in range(args.warm):
        fn()
    eng.profile(1); eng.profile_reset()
    for _ in range(args.reps):
        fn()
    ms, launches, _ = eng.profile_get(scope)
    eng.profile(0)
    return ms / max(launches, 1)


def check_subsample(p, name):
    idx = np.linspace(0, len(p) - 1, 5000).astype(np.int64)
    c = np.ascontiguousarray(p[idx])
    rng = np.random.Generator(np.random.PCG64(5))
    q = np.ascontiguousarray(np.vstack([c[::10] + rng.normal(0, 0.003, size=(500, 3)), rng.uniform(c.min(0) - 0.2, c.max(0) + 0.2, size=(300, 3))]))
    t0 = time.perf_counter()
    srt, srt_self = knnref.sorted_rows(c, q), knnref.sorted_rows(c, c[:800])
    ref_ms = 1e3 * (time.perf_counter() - t0)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([c], None)
        same = all(knnref.same(eng.knn_search(0, q, k, r), knnref.from_sorted(*srt, k, r)) for k, r in ((8, 0.0), (64, 0.0), (16, 0.05), (0, 0.08)))
        got = eng.knn_search(0, None, 33)
        want = knnref.from_sorted(*srt_self, 33, 0.0)
        same = same and got["idx"][:800].tobytes() == want["idx"].tobytes() and got["d2"][:800].tobytes() == want["d2"].tobytes()
    finally:
        eng.close()
    report(what="numpy_reference", case=name, points=5000, ms=ref_ms, gpu_equals_reference=bool(same))
    if not same:
        raise SystemExit("the GPU result differs from tests/knnref.py")


def radius_for(eng, p, target):
    """The radius within which a point of a 2000-point sample has `target` neighbours in the median: the median distance to its
    target-th candidate (itself included)."""
    q = np.ascontiguousarray(p[np.linspace(0, len(p) - 1, 2000).astype(np.int64)])
    d2 = eng.knn_search(0, q, target + 1)["d2"][:, target]
    return float(np.sqrt(np.median(d2)))


def run_case(name, args):
    K, N = SIZES[name]
    p, nr = synth.make_view(0, K, N)
    check_subsample(p, name)
    eng, out_eng, nrm_eng = mvicp.Engine(0), mvicp.Engine(0), mvicp.Engine(0)
    try:
        for e in (eng, out_eng, nrm_eng):
            e.set_frames([p], None)
            e.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        for k in (8, 16, 32, 64):
            split = measure(eng, "self", None, k, 0.0, args, case=name)
            if k <= 32:
                fl = scope_ms(out_eng, lambda: out_eng.lib.mvicp_outlier_filter(out_eng.h, 0, k, -1.0, 0.0, None), "outlier_knn", args)
                report(what="floor_outlier_knn", case=name, k=k, ms_per_call=fl, knn_search_over_floor=split["knn_search"] / fl)
            if k == 16:
                self16 = split["knn_search"]
        for kk in (10, 16):
            ms = scope_ms(nrm_eng, lambda: nrm_eng.recompute_normals(0, kk, want_knn=True), "normals", args)
            report(what="yardstick_normals_kernel", case=name, normals_k=kk, ms_per_call=ms, **({"self16_over_normals16": self16 / ms} if kk == 16 else {}))
        rng = np.random.Generator(np.random.PCG64(17))
        R = synth.so3_exp(np.array([0.004, -0.003, 0.005]))
        moved = np.ascontiguousarray((p - p.mean(0)) @ R.T + p.mean(0) + [0.002, -0.001, 0.0015])
        rand = np.ascontiguousarray(rng.uniform(p.min(0), p.max(0), size=(4096, 3)))
        for label, q in (("queries_moved_cloud", moved), ("queries_random_4096", rand)):
            for order in (1, 0):
                eng.set_option("knn_order", order)
                measure(eng, label, q, 8, 0.0, args, case=name, knn_order=order)
                measure(eng, label, q, 1, 0.0, args, case=name, knn_order=order)
            eng.set_option("knn_order", 1)
            t = timed(eng, lambda: eng.nn_query(0, q), args.warm, args.reps)
            report(what="yardstick_nn_query_wall", case=name, queries=label, m=len(q), **t)
        r30 = radius_for(eng, p, 30)
        measure(eng, "all_self", None, 0, r30, args, case=name)
    finally:
        eng.close(); out_eng.close(); nrm_eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    args = ap.parse_args()
    for name in args.cases.split(","):
        run_case(name, args)


if __name__ == "__main__":
    main()
