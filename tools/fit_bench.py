#!/usr/bin/env python3
"""Times the jet-fitted normals (Engine.fit_normals, csrc/normals_jet.hip) next to mvicp_estimate_normals on the same clouds.

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case, first the result on a 3000-point subsample is compared with the numpy statement of the contract (tests/jetref.py) for both
degrees.  Then, per max_nn = 16 / 30 and ALTERNATING between the three calls so that none has the device to itself for a stretch,
medians of REPS calls after WARM untimed ones of
  mvicp_fit_normals at degree 2 and at degree 3, no radius   the whole call: self-mode search + normals_jet, from a drained stream to its return
  mvicp_estimate_normals at the same max_nn                  the whole call: self-mode search + normals_pca
and the library's own profile scopes (HIP events on its stream): the search's, "normals_jet" and "normals_pca".  Reported: fit / estimate
at equal max_nn for whole calls and for the kernels alone, and the share of rows that kept the PCA normal.  One JSON line per measurement,
on stdout and in --out.

    python tools/fit_bench.py [--cases one200k,one1m] [--reps 7] [--warm 2] [--out profiles/fit_bench.txt]
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
import jetref  # noqa: E402
import mvicp  # noqa: E402
from mvicp import synth  # noqa: E402

KNN_SCOPES = ("knn_key", "knn_search", "knn_count", "knn_fill", "knn_order")
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
            same = jetref.same(eng.fit_normals(0, 16, 0.0, None, degree), jetref.fit(c, 16, 0.0, None, degree))
            report(what="numpy_reference", case=name, points=3000, max_nn=16, degree=degree, gpu_equals_reference=bool(same))
            if not same:
                raise SystemExit("the GPU result differs from tests/jetref.py")
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
    p, _ = synth.make_view(0, K, N)
    check_subsample(p, name)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], None)
        eng.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        n = len(p)
        for k in (16, 30):
            fns = {"estimate": lambda: call(eng, eng.lib.mvicp_estimate_normals, 0, k, 0.0, None),
                   "fit2": lambda: call(eng, eng.lib.mvicp_fit_normals, 0, k, 0.0, None, 2),
                   "fit3": lambda: call(eng, eng.lib.mvicp_fit_normals, 0, k, 0.0, None, 3)}
            times = {key: [] for key in fns}
            for r in range(args.warm + args.reps):   # alternating
                for key, fn in fns.items():
                    t = once(eng, fn)
                    if r >= args.warm:
                        times[key].append(t)
            med = {key: float(np.median(v)) for key, v in times.items()}
            s_est = scopes(eng, fns["estimate"], KNN_SCOPES + ("normals_pca",), args.reps)
            row = dict(what="fit", case=name, n=n, k=k, reps=args.reps, estimate_call_median_ms=med["estimate"],
                       search_scopes_ms=sum(s_est[s] for s in KNN_SCOPES), normals_pca_ms=s_est["normals_pca"])
            for degree in (2, 3):
                key = "fit%d" % degree
                s_fit = scopes(eng, fns[key], ("normals_jet",), args.reps)
                fell_back = int((eng.fit_normals(0, k, 0.0, None, degree, device=True)["fitted"] == 0).sum())
                row.update({key + "_call_median_ms": med[key], key + "_call_min_ms": float(np.min(times[key])),
                            key + "_call_max_ms": float(np.max(times[key])), key + "_over_estimate_call": med[key] / med["estimate"],
                            "normals_jet%d_ms" % degree: s_fit["normals_jet"], "jet%d_over_pca_kernel" % degree: s_fit["normals_jet"] / s_est["normals_pca"],
                            key + "_rows_fell_back": fell_back})
            report(**row)
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.txt"))
    args = ap.parse_args()
    OUT = open(args.out, "w")
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
