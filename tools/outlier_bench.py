#!/usr/bin/env python3
"""Times the outlier filter (Engine.outlier_filter, csrc/outlier.hip) and its yardstick.

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case and k in {8, 16, 32} (std_ratio 2, no radius): first the result on a 5000-point subsample cloud is compared with the numpy statement
of the contract (tests/outlierref.py), whose own time there is printed as context only; then WARM untimed calls and REPS timed ones of
mvicp_outlier_filter, each from a drained stream to the call's return (the call waits for its result; the fetch is not timed): median, min
and max in ms.  The per-pass split comes from the library's own profile scopes ("outlier_knn", "outlier_sum", "outlier_flag",
"outlier_compact": HIP events on its stream) over further calls.
The yardstick is the only other route to the same neighbourhoods: the "normals" scope (the kernel alone) of mvicp_recompute_normals at
min(k + 1, 16) on the same cloud, in the same process, on an engine of its own (it overwrites the frame's normals).  One JSON line per
measurement.

    python tools/outlier_bench.py [--cases one200k,one1m] [--ks 8,16,32] [--reps 7] [--warm 2]
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
import outlierref  # noqa: E402
from mvicp import synth  # noqa: E402

SCOPES = ("outlier_knn", "outlier_sum", "outlier_flag", "outlier_compact")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}


def report(**kw):
    print(json.dumps(kw), flush=True)


def filter_only(eng, k):
    st = eng.lib.mvicp_outlier_filter(eng.h, 0, k, 2.0, 0.0, None)
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


def check_subsample(p, nr, k, name):
    idx = np.linspace(0, len(p) - 1, 5000).astype(np.int64)
    q, qn = np.ascontiguousarray(p[idx]), np.ascontiguousarray(nr[idx])
    t0 = time.perf_counter()
    want = outlierref.outlier_filter(q, qn, k, 2.0, 0.0)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([q], [qn])
        same = outlierref.same(eng.outlier_filter(0, k, 2.0, 0.0), want)
    finally:
        eng.close()
    report(what="numpy_reference", case=name, k=k, points=5000, ms=ref_ms, gpu_equals_reference=same)
    if not same:
        raise SystemExit("the GPU result differs from tests/outlierref.py")


def run_case(name, args):
    K, N = SIZES[name]
    p, nr = synth.make_view(0, K, N)
    eng, yard = mvicp.Engine(0), mvicp.Engine(0)
    try:
        eng.set_frames([p], [nr]); yard.set_frames([p], None)
        eng.get_structure(0, "scalars"); yard.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        for k in args.ks:
            check_subsample(p, nr, k, name)
            t = timed(eng, lambda: filter_only(eng, k), args.warm, args.reps)
            kept = filter_only(eng, k)
            report(what="outlier_filter", case=name, points=N, k=k, std_ratio=2.0, kept=int(kept), **t)
            eng.profile(1); eng.profile_reset()
            for _ in range(args.reps):
                filter_only(eng, k)
            split = {s: eng.profile_get(s)[0] / args.reps for s in SCOPES}
            eng.profile(0)
            report(what="split_ms_per_call", case=name, k=k, kernels_ms=sum(split.values()), **split)
            kk = min(k + 1, 16)
            for _ in range(args.warm):
                yard.recompute_normals(0, kk)
            yard.profile(1); yard.profile_reset()
            for _ in range(args.reps):
                yard.recompute_normals(0, kk)
            ms, launches, _ = yard.profile_get("normals")
            yard.profile(0)
            report(what="yardstick_normals_kernel", case=name, k=k, normals_k=kk, ms_per_call=ms / max(launches, 1), launches=int(launches),
                   knn_over_normals=split["outlier_knn"] / (ms / max(launches, 1)))
    finally:
        eng.close(); yard.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    args = ap.parse_args()
    args.ks = [int(v) for v in args.ks.split(",")]
    for name in args.cases.split(","):
        run_case(name, args)


if __name__ == "__main__":
    main()
