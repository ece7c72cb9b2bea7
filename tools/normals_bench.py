#!/usr/bin/env python3
"""Times the exactly specified normals (Engine.estimate_normals, csrc/normals_pca.hip) next to mvicp_recompute_normals on the same clouds.

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case, first the result on a 3000-point subsample is compared with the numpy statement of the contract (tests/normref.py).  Then,
ALTERNATING between the two so that neither has the device to itself for a stretch, medians of REPS calls after WARM untimed ones of
  mvicp_estimate_normals at max_nn = 10 / 16 / 30, no radius   the whole call: self-mode search + normals_pca, from a drained stream to its return
  mvicp_recompute_normals at k = 10 / 16                       the whole call (k <= 16 is its limit), no host destination
and the library's own profile scopes (HIP events on its stream): the search's ("knn_key", "knn_search", "knn_count", "knn_fill",
"knn_order"), "normals_pca" and "normals".  Reported: estimate / recompute at equal k (whole calls and scopes), and for normals_pca its
own byte model -- per point its position, count and index row and the 36 bytes it writes, per row entry one position of 24 bytes -- as a
share of the MI355X's 8 TB/s HBM peak.  One JSON line per measurement, on stdout and in --out.

    python tools/normals_bench.py [--cases one200k,one1m] [--reps 7] [--warm 2] [--out profiles/normals_bench.txt]
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
import normref  # noqa: E402
from mvicp import synth  # noqa: E402

KNN_SCOPES = ("knn_key", "knn_search", "knn_count", "knn_fill", "knn_order")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}
HBM_PEAK = 8.0e12
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
    t0 = time.perf_counter()
    want = normref.normals(c, 16, 0.0, (0.0, 0.0, 0.0))
    ref_ms = 1e3 * (time.perf_counter() - t0)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([c], None)
        same = normref.same(eng.estimate_normals(0, 16), want)
    finally:
        eng.close()
    report(what="numpy_reference", case=name, points=3000, max_nn=16, reference_ms=ref_ms, gpu_equals_reference=bool(same))
    if not same:
        raise SystemExit("the GPU result differs from tests/normref.py")


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
        for k in (10, 16, 30):
            est = lambda: call(eng, eng.lib.mvicp_estimate_normals, 0, k, 0.0, None)
            rec = (lambda: call(eng, eng.lib.mvicp_recompute_normals, 0, k, None, None)) if k <= 16 else None
            t_est, t_rec = [], []
            for r in range(args.warm + args.reps):   # alternating
                a = once(eng, est)
                b = once(eng, rec) if rec else None
                if r >= args.warm:
                    t_est.append(a)
                    if rec:
                        t_rec.append(b)
            entries = n * k
            s_est = scopes(eng, est, KNN_SCOPES + ("normals_pca",), args.reps)
            search_ms = sum(s_est[s] for s in KNN_SCOPES)
            pca_bytes = (24 + 4 + 4 * k + 36) * n + 24 * entries
            row = dict(what="normals", case=name, n=n, k=k, reps=args.reps, estimate_call_median_ms=float(np.median(t_est)),
                       estimate_call_min_ms=float(np.min(t_est)), estimate_call_max_ms=float(np.max(t_est)),
                       search_scopes_ms=search_ms, normals_pca_ms=s_est["normals_pca"], pca_over_search=s_est["normals_pca"] / search_ms,
                       pca_model_bytes=pca_bytes, pca_implied_GBps=pca_bytes / (s_est["normals_pca"] * 1e-3) / 1e9,
                       pca_share_of_hbm_peak=pca_bytes / (s_est["normals_pca"] * 1e-3) / HBM_PEAK)
            if rec:
                s_rec = scopes(eng, rec, ("normals",), args.reps)
                row.update(recompute_call_median_ms=float(np.median(t_rec)), recompute_call_min_ms=float(np.min(t_rec)),
                           recompute_call_max_ms=float(np.max(t_rec)), normals_scope_ms=s_rec["normals"],
                           estimate_over_recompute_call=float(np.median(t_est) / np.median(t_rec)),
                           estimate_over_recompute_scopes=(search_ms + s_est["normals_pca"]) / s_rec["normals"],
                           search_over_normals_scope=search_ms / s_rec["normals"])
            report(**row)
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.txt"))
    args = ap.parse_args()
    OUT = open(args.out, "w")
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
