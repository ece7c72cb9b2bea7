#!/usr/bin/env python3
"""Times jet smoothing (Engine.smooth_points, csrc/smooth.hip) next to mvicp_fit_normals at the same arguments on the same clouds.

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case, first the result on a 3000-point subsample is compared with the numpy statement of the contract (tests/smoothref.py) for both
degrees.  Then, per (max_nn, degree) = (16, 2), (30, 2), (16, 3) and ALTERNATING between the two calls so that neither has the device to
itself for a stretch, medians of REPS calls after WARM untimed ones of
  mvicp_smooth_points, no radius, no limit   the whole call: self-mode search + jet_smooth, from a drained stream to its return
  mvicp_fit_normals at the same arguments    the whole call: self-mode search + normals_jet
and the library's own profile scopes (HIP events on its stream): the search's, "jet_smooth" and "normals_jet".  The yardstick is the fit in
the same process: the call does the same search and the same factorisation, plus one substitution row and 49 more bytes written per point
(86 against 37).  Reported: smooth / fit for whole calls and for the kernels alone, and the bytes each kernel moves by its own count.  One
JSON line per measurement, on stdout and in --out.

    python tools/smooth_bench.py [--cases one200k,one1m] [--reps 7] [--warm 2] [--out profiles/smooth_bench.txt]
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
import smoothref  # noqa: E402
from mvicp import synth  # noqa: E402

KNN_SCOPES = ("knn_key", "knn_search", "knn_count", "knn_fill", "knn_order")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}
SETTINGS = ((16, 2), (30, 2), (16, 3))
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


def check_subsample(p, name):
    c = np.ascontiguousarray(p[np.linspace(0, len(p) - 1, 3000).astype(np.int64)])
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([c], None)
        for degree in (2, 3):
            same = smoothref.same(eng.smooth_points(0, 16, 0.0, None, degree), smoothref.smooth(c, 16, 0.0, None, degree, 0.0))
            report(what="numpy_reference", case=name, points=3000, max_nn=16, degree=degree, gpu_equals_reference=bool(same))
            if not same:
                raise SystemExit("the GPU result differs from tests/smoothref.py")
    finally:
        eng.close()


def scopes(eng, fn, names, reps):
    eng.profile(1); eng.profile_reset()
    for _ in range(reps):
        fn()
    out = {s: eng.profile_get(s) for s in names}
    eng.profile(0)
    return {s: v[0] / reps for s, v in out.items()}, {s: v[2] / reps if len(v) > 2 else None for s, v in out.items()}


def run_case(name, args):
    K, N = SIZES[name]
    p, _ = synth.make_view(0, K, N)
    check_subsample(p, name)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], None)
        eng.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        n = len(p)
        for k, degree in SETTINGS:
            fns = {"fit": lambda: call(eng, eng.lib.mvicp_fit_normals, 0, k, 0.0, None, degree),
                   "smooth": lambda: call(eng, eng.lib.mvicp_smooth_points, 0, k, 0.0, None, degree, 0.0)}
            times = {key: [] for key in fns}
            for r in range(args.warm + args.reps):   # alternating
                for key, fn in fns.items():
                    t = once(eng, fn)
                    if r >= args.warm:
                        times[key].append(t)
            med = {key: float(np.median(v)) for key, v in times.items()}
            s_fit, b_fit = scopes(eng, fns["fit"], KNN_SCOPES + ("normals_jet",), args.reps)
            s_smo, b_smo = scopes(eng, fns["smooth"], KNN_SCOPES + ("jet_smooth",), args.reps)
            res = eng.smooth_points(0, k, 0.0, None, degree, device=True)
            report(what="smooth", case=name, n=n, k=k, degree=degree, reps=args.reps,
                   fit_call_median_ms=med["fit"], fit_call_min_ms=float(np.min(times["fit"])), fit_call_max_ms=float(np.max(times["fit"])),
                   smooth_call_median_ms=med["smooth"], smooth_call_min_ms=float(np.min(times["smooth"])), smooth_call_max_ms=float(np.max(times["smooth"])),
                   smooth_over_fit_call=med["smooth"] / med["fit"],
                   search_scopes_ms=sum(s_fit[s] for s in KNN_SCOPES), search_scopes_smooth_ms=sum(s_smo[s] for s in KNN_SCOPES),
                   normals_jet_ms=s_fit["normals_jet"], jet_smooth_ms=s_smo["jet_smooth"], smooth_over_jet_kernel=s_smo["jet_smooth"] / s_fit["normals_jet"],
                   normals_jet_bytes=b_fit["normals_jet"], jet_smooth_bytes=b_smo["jet_smooth"],
                   rows_fell_back=int((res["fitted"] == 0).sum()), rows_moved=int(res["moved"].sum()))
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.txt"))
    args = ap.parse_args()
    OUT = open(args.out, "w")
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
