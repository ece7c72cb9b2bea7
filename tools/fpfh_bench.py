#!/usr/bin/env python3
"""Times the FPFH descriptors (Engine.fpfh, csrc/fpfh.hip) and the neighbour search they ride on.

  one200k : one synthetic view of 200 000 points with its normals
  one1m   : one synthetic view of 1 000 000 points with its normals

Per case, first the result on a 3000-point subsample is compared with the numpy statement of the contract (tests/fpfhref.py), both
timed: the whole GPU call against the reference.  Then, at max_nn = 16 / 32 / 64 and the radius whose rows hold about 30 neighbours (the
median distance to the 31st candidate over a sample of rows, as tools/knn_bench.py derives it), WARM untimed and REPS timed calls of
  mvicp_fpfh                        the whole call: search + SPFH pass + sum pass, from a drained stream to the call's return
  mvicp_knn_search (self mode)      the same k and radius, same engine, same process: what the descriptor passes ride on
and the library's own profile scopes ("knn_search", "fpfh_spfh", "fpfh_sum": HIP events on its stream) over further calls.  Each pass is
reported as a ratio of the "knn_search" scope of the same calls.  Next to pass 2 its algorithmic bytes -- per point cnt (4), its own 33
counts and r (41) and the 33 doubles written (264); per row entry idx and d2 (12); per neighbour 33 count bytes and r (41) -- and the
bandwidth they imply.  One JSON line per measurement, on stdout and in --out.

    python tools/fpfh_bench.py [--cases one200k,one1m] [--reps 7] [--warm 2] [--out profiles/fpfh_bench.txt]
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
import fpfhref  # noqa: E402
import knnref  # noqa: E402
from mvicp import synth  # noqa: E402

SCOPES = ("knn_search", "fpfh_spfh", "fpfh_sum")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}
OUT = None


def report(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def call(eng, fn, *a):
    st = fn(eng.h, *a)
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


def check_subsample(p, nr, name, args):
    idx = np.linspace(0, len(p) - 1, 3000).astype(np.int64)
    c, cn = np.ascontiguousarray(p[idx]), np.ascontiguousarray(nr[idx])
    radius = float(np.sqrt(np.median(knnref.sorted_rows(c, c[::10])[1][:, 30])))
    t0 = time.perf_counter()
    want = fpfhref.fpfh(c, cn, radius, 32)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([c], [cn])
        eng.get_structure(0, "scalars")
        got = eng.fpfh(0, radius, 32)
        same = fpfhref.same(got, want, keys=("desc", "used"))
        t = timed(eng, lambda: call(eng, eng.lib.mvicp_fpfh, 0, radius, 32), args.warm, args.reps)
    finally:
        eng.close()
    report(what="numpy_reference", case=name, points=3000, max_nn=32, radius=radius, reference_ms=ref_ms, gpu_call_median_ms=t["median_ms"],
           reference_over_gpu_call=ref_ms / t["median_ms"], gpu_equals_reference=bool(same))
    if not same:
        raise SystemExit("the GPU result differs from tests/fpfhref.py")


def radius_for(eng, p, target):
    q = np.ascontiguousarray(p[np.linspace(0, len(p) - 1, 2000).astype(np.int64)])
    d2 = eng.knn_search(0, q, target + 1)["d2"][:, target]
    return float(np.sqrt(np.median(d2)))


def run_case(name, args):
    K, N = SIZES[name]
    p, nr = synth.make_view(0, K, N)
    check_subsample(p, nr, name, args)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], [nr])
        eng.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        n = len(p)
        r30 = radius_for(eng, p, 30)
        for k in (16, 32, 64):
            fp = lambda: call(eng, eng.lib.mvicp_fpfh, 0, r30, k)
            kn = lambda: call(eng, eng.lib.mvicp_knn_search, 0, None, 0, k, r30)
            t_kn = timed(eng, kn, args.warm, args.reps)
            t_fp = timed(eng, fp, args.warm, args.reps)
            used = eng.fpfh(0, r30, k)["used"]
            entries, neighbours = int(kn()), int(used.sum(dtype=np.int64))
            eng.profile(1); eng.profile_reset()
            for _ in range(args.reps):
                fp()
            split = {s: eng.profile_get(s)[0] / args.reps for s in SCOPES}
            eng.profile(0)
            bytes2 = (4 + 41 + 264) * n + 12 * entries + 41 * neighbours
            report(what="fpfh", case=name, n=n, max_nn=k, radius=r30, entries=entries, neighbours=neighbours, mean_neighbours=neighbours / n,
                   call_median_ms=t_fp["median_ms"], call_min_ms=t_fp["min_ms"], call_max_ms=t_fp["max_ms"],
                   knn_call_median_ms=t_kn["median_ms"], knn_call_min_ms=t_kn["min_ms"], knn_call_max_ms=t_kn["max_ms"], reps=args.reps,
                   call_over_knn_call=t_fp["median_ms"] / t_kn["median_ms"],
                   knn_search_ms=split["knn_search"], fpfh_spfh_ms=split["fpfh_spfh"], fpfh_sum_ms=split["fpfh_sum"],
                   spfh_over_knn_search=split["fpfh_spfh"] / split["knn_search"], sum_over_knn_search=split["fpfh_sum"] / split["knn_search"],
                   passes_over_knn_search=(split["fpfh_spfh"] + split["fpfh_sum"]) / split["knn_search"],
                   sum_algorithmic_bytes=bytes2, sum_implied_GBps=bytes2 / (split["fpfh_sum"] * 1e-3) / 1e9)
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_bench.txt"))
    args = ap.parse_args()
    OUT = open(args.out, "w")
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
