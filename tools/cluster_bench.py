#!/usr/bin/env python3
"""Times the clustering stage (Engine.cluster, csrc/cluster.hip) next to the two earlier routes to a radius neighbourhood.

  one200k : one synthetic view of 200 000 points (the bench surface)
  one1m   : one synthetic view of 1 000 000 points

Per case and k in {8, 16, 30}: the radius is the median k-th neighbour distance of the cloud (a k-distance query of mvicp_outlier_filter
with both rules off), so a point has about k neighbours within it.  First the result on a 4000-point subsample at the subsample's own
radius is compared with the numpy statement of the contract (tests/clusterref.py).  Then, after WARM untimed rounds, REPS rounds that
ALTERNATE three calls, each timed from a drained stream to the call's return (every call waits for its result; no fetch is timed):
  cluster       mvicp_cluster(radius, min_pts 4)
  outlier       mvicp_outlier_filter(k, statistical rule off, radius): the radius rule at the matching k -- the floor of ONE traversal
  knn_all       mvicp_knn_search(self mode, k = 0, radius): every neighbour within the radius in CSR form -- what a caller would need
                before clustering on the host
Medians, minima and maxima in ms, the ratios of the medians, and the per-scope kernel times of the cluster call from the library's own
profile scopes (HIP events on its stream) over further calls; mvicp_cluster_select(min_size 100) is timed the same way.  One JSON line
per measurement, to stdout and to --out (default profiles/cluster_bench.txt).  No time is asserted.

    python tools/cluster_bench.py [--cases one200k,one1m] [--ks 8,16,30] [--reps 7] [--warm 2] [--out FILE]
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
import clusterref  # noqa: E402
import mvicp  # noqa: E402
from mvicp import synth  # noqa: E402

SCOPES = ("cluster_core", "cluster_union", "cluster_border", "cluster_label", "cluster_compact")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}
MIN_PTS = 4
OUT = None


def report(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n"); OUT.flush()


def must(eng, st):
    if st < 0:
        raise SystemExit(eng.lib.mvicp_last_error().decode())
    return st


def k_radius(eng, k):
    """The median distance to the k-th neighbour (the point itself not counted) of frame 0."""
    r = eng.outlier_filter(0, k, -1.0, 0.0)
    return float(np.sqrt(np.median(r["kd2"])))


def stats(ms):
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": len(ms)}


def check_subsample(p, nr, k, name):
    idx = np.linspace(0, len(p) - 1, 4000).astype(np.int64)
    q, qn = np.ascontiguousarray(p[idx]), np.ascontiguousarray(nr[idx])
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([q], [qn])
        radius = k_radius(eng, k)
        t0 = time.perf_counter()
        want = clusterref.cluster(q, qn, radius, MIN_PTS)
        ref_ms = 1e3 * (time.perf_counter() - t0)
        got = eng.cluster(0, radius, MIN_PTS)
        same = clusterref.same(got, want) and clusterref.same_kept(eng.cluster_select(100, 0), clusterref.select(q, qn, want, 100, 0))
    finally:
        eng.close()
    report(what="numpy_reference", case=name, k=k, points=4000, radius=radius, ms=ref_ms, stats=want["stats"], gpu_equals_reference=same)
    if not same:
        raise SystemExit("the GPU result differs from tests/clusterref.py")


def run_case(name, args):
    K, N = SIZES[name]
    p, nr = synth.make_view(0, K, N)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], [nr])
        eng.get_structure(0, "scalars")   # waits for the structure build: nothing else runs while the calls are timed
        lib, h = eng.lib, eng.h
        for k in args.ks:
            check_subsample(p, nr, k, name)
            radius = k_radius(eng, k)
            calls = {
                "cluster": lambda: must(eng, lib.mvicp_cluster(h, 0, radius, MIN_PTS, None)),
                "outlier": lambda: must(eng, lib.mvicp_outlier_filter(h, 0, k, -1.0, radius, None)),
                "knn_all": lambda: must(eng, lib.mvicp_knn_search(h, 0, None, 0, 0, radius)),
            }
            ms = {key: [] for key in calls}
            out = {}
            for r in range(args.warm + args.reps):
                for key, fn in calls.items():
                    eng.sync()
                    t0 = time.perf_counter()
                    out[key] = fn()
                    t1 = time.perf_counter()
                    if r >= args.warm:
                        ms[key].append(1e3 * (t1 - t0))
            t = {key: stats(v) for key, v in ms.items()}
            S = mvicp.lib.ClusterStats()
            must(eng, lib.mvicp_cluster(h, 0, radius, MIN_PTS, S))
            report(what="cluster", case=name, points=N, k=k, radius=radius, min_pts=MIN_PTS, stats=S.as_dict(), **t["cluster"])
            report(what="baseline_outlier_radius_rule", case=name, k=k, radius=radius, kept=int(out["outlier"]), **t["outlier"])
            report(what="baseline_knn_all", case=name, k=k, radius=radius, entries=int(out["knn_all"]), entries_per_point=out["knn_all"] / N, **t["knn_all"])
            report(what="ratios_of_medians", case=name, k=k, cluster_over_outlier=t["cluster"]["median_ms"] / t["outlier"]["median_ms"],
                   cluster_over_knn_all=t["cluster"]["median_ms"] / t["knn_all"]["median_ms"])
            sel = []
            for r in range(args.warm + args.reps):
                eng.sync()
                t0 = time.perf_counter()
                kept = must(eng, lib.mvicp_cluster_select(h, 100, 0))
                if r >= args.warm:
                    sel.append(1e3 * (time.perf_counter() - t0))
            report(what="cluster_select", case=name, k=k, min_size=100, kept=int(kept), **stats(sel))
            eng.profile(1); eng.profile_reset()
            for _ in range(args.reps):
                must(eng, lib.mvicp_cluster(h, 0, radius, MIN_PTS, None))
                must(eng, lib.mvicp_cluster_select(h, 100, 0))
            split = {s: eng.profile_get(s)[0] / args.reps for s in SCOPES}
            eng.profile(0)
            report(what="split_ms_per_call", case=name, k=k, kernels_ms=sum(split.values()), **split)
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--ks", default="8,16,30")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_bench.txt"))
    args = ap.parse_args()
    args.ks = [int(v) for v in args.ks.split(",")]
    OUT = open(args.out, "w")
    OUT.write("# tools/cluster_bench.py on one MI355X (gfx950): the clustering stage (mvicp_cluster, DESIGN.md section 3.18), min_pts %d\n"
              "# radius = the median k-th neighbour distance of the cloud; %d warm + %d timed rounds that alternate cluster / outlier (radius rule at k) /\n"
              "# knn_all (mvicp_knn_search self mode, k = 0), wall ms from a drained stream to the call's return; split_ms_per_call: the library's\n"
              "# profile scopes (HIP events) over %d further calls of mvicp_cluster + mvicp_cluster_select; numpy_reference: tests/clusterref.py on the\n"
              "# 4000-point subsample the GPU result is compared with first (context only).\n" % (MIN_PTS, args.warm, args.reps, args.reps))
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
