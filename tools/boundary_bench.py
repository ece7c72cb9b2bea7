#!/usr/bin/env python3
"""Times the boundary stage (Engine.boundary, csrc/boundary.hip) next to mvicp_estimate_normals on the same clouds, and one registration
round without rejection, with Engine.reject_correspondences (the host route) and with Engine.set_reject_mask (the mask inside the search).

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case, first the result on a 3000-point subsample is compared with the numpy statement of the contract (tests/boundref.py).  Then, per
max_nn = 16 / 30 and ALTERNATING between the two calls so that neither has the device to itself for a stretch, medians of REPS calls
after WARM untimed ones of
  mvicp_boundary at cos_gap = -0.5, no radius, source 0    the whole call: self-mode search + boundary, from a drained stream to its return
  mvicp_estimate_normals at the same max_nn                the whole call: self-mode search + normals_pca
and the library's own profile scopes (HIP events on its stream): the search's, "boundary" and "normals_pca".  Reported: boundary / estimate
at equal max_nn for whole calls and for the kernels alone, the points flagged, and mvicp_boundary_select.

The round: bench-like problems of 4 views; per round mvicp_correspond + mvicp_optimize (point-to-plane, robust) in three legs, alternating,
on an engine each; medians of REPS rounds: "plain" (no rejection), "reject" (the host route: reject_correspondences(target masks) between
the search and the solve) and "device" (the same masks handed to the search once, set_reject_mask(i, mask, REJECT_AS_TARGET), nothing per
round).  Twice: a FIRST round (from the start poses after reset_history: a first search in every leg, so the host leg's difference is the
lists' two trips through the host and the lost queued evaluation) and LATER rounds (the loop continued: the plain and the device leg settle
into cached and fixed-point rounds, the host leg searches like a first round every time).  The yardstick of the device leg is the plain
leg of the same run.

One JSON line per measurement, on stdout and in --out.

    python tools/boundary_bench.py [--cases one200k,one1m | --cases none] [--reps 7] [--warm 2] [--out profiles/boundary_bench.txt]
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
import boundref  # noqa: E402
import mvicp  # noqa: E402
from mvicp import lib as L  # noqa: E402
from mvicp import synth  # noqa: E402

KNN_SCOPES = ("knn_key", "knn_search", "knn_count", "knn_fill", "knn_order")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}
ROUND_SIZES = (20_000, 200_000)
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


def once(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def check_subsample(p, nrm, name):
    at = np.linspace(0, len(p) - 1, 3000).astype(np.int64)
    c, cn = np.ascontiguousarray(p[at]), np.ascontiguousarray(nrm[at])
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([c], [cn])
        for k, cos_gap in ((16, -0.5), (30, -0.5), (30, 0.0)):
            want = boundref.boundary(c, cn, k, 0.0, cos_gap)
            same = boundref.same(eng.boundary(0, k, 0.0, cos_gap), want)
            report(what="numpy_reference", case=name, points=3000, max_nn=k, cos_gap=cos_gap, flagged=int(want["boundary"]), gpu_equals_reference=bool(same))
            if not same:
                raise SystemExit("the GPU result differs from tests/boundref.py")
    finally:
        eng.close()


def scopes(eng, fn, names, reps):
    eng.profile(1); eng.profile_reset()
    for _ in range(reps):
        fn()
    out = {s: eng.profile_get(s)[0] / reps for s in names}
    eng.profile(0)
    return out


def run_case(name, args):
    K, N = SIZES[name]
    p, nrm = synth.make_view(0, K, N)
    check_subsample(p, nrm, name)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], [nrm])
        eng.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        n = len(p)
        for k in (16, 30):
            fns = {"estimate": lambda: call(eng, eng.lib.mvicp_estimate_normals, 0, k, 0.0, None),
                   "boundary": lambda: call(eng, eng.lib.mvicp_boundary, 0, 0, k, 0.0, -0.5)}
            times = {key: [] for key in fns}
            for r in range(args.warm + args.reps):   # alternating
                for key, fn in fns.items():
                    t = once(eng, fn)
                    if r >= args.warm:
                        times[key].append(t)
            med = {key: float(np.median(v)) for key, v in times.items()}
            s_est = scopes(eng, fns["estimate"], KNN_SCOPES + ("normals_pca",), args.reps)
            s_bnd = scopes(eng, fns["boundary"], KNN_SCOPES + ("boundary",), args.reps)
            flagged = int(fns["boundary"]())
            sel = [once(eng, lambda: call(eng, eng.lib.mvicp_boundary_select, 0)) for _ in range(args.warm + args.reps)][args.warm:]
            report(what="boundary", case=name, n=n, k=k, cos_gap=-0.5, reps=args.reps, flagged=flagged,
                   boundary_call_median_ms=med["boundary"], boundary_call_min_ms=float(np.min(times["boundary"])), boundary_call_max_ms=float(np.max(times["boundary"])),
                   estimate_call_median_ms=med["estimate"], estimate_call_min_ms=float(np.min(times["estimate"])), estimate_call_max_ms=float(np.max(times["estimate"])),
                   boundary_over_estimate_call=med["boundary"] / med["estimate"],
                   search_scopes_ms=sum(s_bnd[s] for s in KNN_SCOPES), boundary_kernel_ms=s_bnd["boundary"], normals_pca_ms=s_est["normals_pca"],
                   boundary_over_pca_kernel=s_bnd["boundary"] / s_est["normals_pca"], select_rest_median_ms=float(np.median(sel)))
    finally:
        eng.close()


def run_round(N, args):
    """one registration round in three legs -- plain, rejecting on the host, mask inside the search --, alternating, each from the same start on an
    engine of its own"""
    pb = synth.make_problem(4, N)
    engines = {}
    try:
        for key in ("plain", "reject", "device"):
            e = mvicp.Engine(0)
            e.set_frames(pb["pts"], pb["nor"])
            engines[key] = e
        masks = [engines["reject"].boundary(i, 30)["flag"] for i in range(4)]
        for i in range(4):   # once, before the graph: nothing of this leg is called per round
            engines["device"].set_reject_mask(i, masks[i], L.REJECT_AS_TARGET)
        for e in engines.values():
            e.set_graph(pb["src"], pb["dst"])
        poses = {key: pb["init"].copy() for key in engines}
        times, dropped = {key: [] for key in engines}, []

        def one(key):
            e = engines[key]
            e.correspond(poses[key], pb["fixed"], 0.05)
            if key == "reject":
                dropped.append(int(e.reject_correspondences(masks).sum()))
            poses[key], _ = e.optimize(poses[key], pb["fixed"], L.PARAM_SOPHUS_SE3, True, True, 50)

        # a FIRST round: both legs from the start poses with no history (every search is a first search in both)
        first = {key: [] for key in engines}
        for r in range(args.warm + args.reps):
            for key in engines:
                engines[key].reset_history()
                poses[key] = pb["init"].copy()
                t = once(engines[key], lambda: one(key))
                if r >= args.warm:
                    first[key].append(t)
        # LATER rounds: the loop goes on from its own poses; the plain leg settles into cached, then fixed-point rounds, the rejecting leg cannot
        for r in range(args.warm + args.reps):
            for key in engines:
                t = once(engines[key], lambda: one(key))
                if r >= args.warm:
                    times[key].append(t)
        med = {key: float(np.median(v)) for key, v in times.items()}
        med1 = {key: float(np.median(v)) for key, v in first.items()}
        report(what="round", views=4, points_per_view=N, reps=args.reps, flagged=[int(m.sum()) for m in masks], dropped_last_round=dropped[-1],
               pairs_last_round=int(engines["plain"].counts.sum()),
               first_plain_median_ms=med1["plain"], first_plain_min_ms=float(np.min(first["plain"])), first_plain_max_ms=float(np.max(first["plain"])),
               first_reject_median_ms=med1["reject"], first_reject_min_ms=float(np.min(first["reject"])), first_reject_max_ms=float(np.max(first["reject"])),
               first_reject_over_plain=med1["reject"] / med1["plain"],
               later_plain_median_ms=med["plain"], later_plain_min_ms=float(np.min(times["plain"])), later_plain_max_ms=float(np.max(times["plain"])),
               later_reject_median_ms=med["reject"], later_reject_min_ms=float(np.min(times["reject"])), later_reject_max_ms=float(np.max(times["reject"])),
               later_reject_over_plain=med["reject"] / med["plain"],
               first_device_median_ms=med1["device"], first_device_min_ms=float(np.min(first["device"])), first_device_max_ms=float(np.max(first["device"])),
               first_device_over_plain=med1["device"] / med1["plain"],
               later_device_median_ms=med["device"], later_device_min_ms=float(np.min(times["device"])), later_device_max_ms=float(np.max(times["device"])),
               later_device_over_plain=med["device"] / med["plain"], later_device_over_reject=med["device"] / med["reject"],
               pairs_last_round_device=int(engines["device"].counts.sum()))
    finally:
        for e in engines.values():
            e.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.txt"))
    args = ap.parse_args()
    OUT = open(args.out, "w")
    for name in args.cases.split(","):
        if name and name != "none":   # (--cases none: the rounds alone)
            run_case(name, args)
    for N in ROUND_SIZES:
        run_round(N, args)
    OUT.close()


if __name__ == "__main__":
    main()
