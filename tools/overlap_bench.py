#!/usr/bin/env python3
"""Times the overlap census (Engine.overlap, csrc/overlap.hip) and the work-around it replaces.

  census     : cfg4 (32 x 200 k) and cfg5 (64 x 1 M) sizes, initial poses, max_samples 4096 and 0
  workaround : K = 8, N = 100 000 — all 56 ordered pairs through set_graph + ONE first-round correspond (the graph's set-up is not
               counted; reset_history before every repetition so that each is a first round), next to the census at max_samples
               4096 and 0 on the same clouds; checks hits == counts there.

Every figure: WARM untimed repetitions, then REPS timed ones, each from a drained stream (Engine.sync) to the call's return (the
census and the search both wait for their own results); median, min and max are printed.  One JSON line per measurement.

    python tools/overlap_bench.py [--what census,workaround] [--sizes cfg4,cfg5] [--reps 7] [--warm 2] [--thresh 0.05]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
import mvicp  # noqa: E402
from mvicp import lib as L  # noqa: E402
from mvicp import synth  # noqa: E402

SIZES = {"cfg4": (32, 200_000), "cfg5": (64, 1_000_000)}


def timed(eng, fn, warm, reps, before=None):
    ms = []
    for r in range(warm + reps):
        if before:
            before()
        eng.sync()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if r >= warm:
            ms.append(1e3 * (t1 - t0))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps}


def report(**kw):
    print(json.dumps(kw), flush=True)


def census(name, args):
    K, N = SIZES[name]
    poses = synth.make_poses(K)
    eng = mvicp.Engine(0)
    try:
        eng.lib.mvicp_set_num_frames(eng.h, K)
        eng.n_frames = K; eng.npts = [0] * K
        for k in range(K):   # one view at a time: cfg5 is 1.5 GB of host points
            p, _ = synth.make_view(k, K, N)
            eng.set_frame(k, p)
        eng.get_structure(0, "scalars")   # waits for the structure builds
        for ms in (4096, 0):
            out = {}
            t = timed(eng, lambda: out.update(eng.overlap(poses["init"], args.thresh, ms)), args.warm, args.reps)
            q = int(out["samples"].sum()) * (K - 1)
            report(what="census", size=name, K=K, N=N, max_samples=ms, thresh=args.thresh, queries=q,
                   pairs_with_hits=int((out["hits"] > 0).sum() - K), **t)
    finally:
        eng.close()


def workaround(args):
    K, N = 8, 100_000
    pb = synth.make_problem(K, N)
    src = np.array([i for i in range(K) for j in range(K) if i != j], dtype=np.int32)
    dst = np.array([j for i in range(K) for j in range(K) if i != j], dtype=np.int32)
    nofixed = np.zeros(K, dtype=np.uint8)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        res = {}
        for ms in (4096, 0):
            out = {}
            res[ms] = timed(eng, lambda: out.update(eng.overlap(pb["init"], args.thresh, ms)), args.warm, args.reps)
            report(what="census", size="K8_N100k", K=K, N=N, max_samples=ms, thresh=args.thresh, **res[ms])
            if ms == 0:
                full = out
        eng.set_graph(src, dst)
        got = {}
        t = timed(eng, lambda: got.update(counts=eng.correspond(pb["init"], nofixed, args.thresh)[0]), args.warm, args.reps, before=eng.reset_history)
        report(what="workaround", size="K8_N100k", K=K, N=N, edges=len(src), thresh=args.thresh, **t)
        same = bool(np.array_equal(got["counts"], full["hits"][src, dst]))
        report(what="check", hits_equal_counts=same,
               speedup_4096=t["median_ms"] / res[4096]["median_ms"], speedup_all_points=t["median_ms"] / res[0]["median_ms"],
               worst_case_speedup_4096=t["min_ms"] / res[4096]["max_ms"])
        if not same:
            raise SystemExit("census hits differ from the work-around's counts")
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="census,workaround")
    ap.add_argument("--sizes", default="cfg4,cfg5")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--thresh", type=float, default=0.05)
    args = ap.parse_args()
    what = args.what.split(",")
    if "workaround" in what:
        workaround(args)
    if "census" in what:
        for name in args.sizes.split(","):
            census(name, args)


if __name__ == "__main__":
    main()
