#!/usr/bin/env python3
"""Times the viewpoint-free orientation (Engine.orient_normals, csrc/orient.hip) next to mvicp_estimate_normals at the same k on the same clouds.

  one200k : one synthetic view of 200 000 points
  one1m   : one synthetic view of 1 000 000 points

Per case, first the result on a 3000-point subsample is compared with the numpy statement of the contract (tests/orientref.py).  Then the
normals of the cloud are estimated at max_nn = 16 and adopted with every point's sign scrambled at random, and, ALTERNATING between the two
so that neither has the device to itself for a stretch, medians of REPS calls after WARM untimed ones of
  mvicp_orient_normals at k = 10 / 16, no radius, source 0, MVICP_ORIENT_ANCHOR   the whole call: self-mode search + rounds + finish
  mvicp_estimate_normals at the same k                                             the whole call: self-mode search + normals_pca
and the library's own profile scopes (HIP events on its stream): the search's, "orient_round", "orient_finish" and "normals_pca".  The
"orient_round" scope is opened twice per Boruvka round -- around the four kernels of the round and around each jump launch -- so its
count per call is twice the number of rounds when one jump launch per round suffices.  One JSON line per measurement, on stdout and in
--out.

    python tools/orient_bench.py [--cases one200k,one1m] [--reps 7] [--warm 2] [--out profiles/orient_bench.txt]
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
import orientref  # noqa: E402
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


def scrambled(nrm, seed):
    s = np.where(np.random.default_rng(seed).integers(0, 2, len(nrm)) == 1, -1.0, 1.0)
    return np.ascontiguousarray(nrm * s[:, None])


def check_subsample(p, name):
    c = np.ascontiguousarray(p[np.linspace(0, len(p) - 1, 3000).astype(np.int64)])
    N = scrambled(normref.normals(c, 16)["nrm"], 1)
    t0 = time.perf_counter()
    want = orientref.orient(c, N, 10)
    ref_ms = 1e3 * (time.perf_counter() - t0)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([c], [N])
        same = orientref.same(eng.orient_normals(0, 10), want)
    finally:
        eng.close()
    report(what="numpy_reference", case=name, points=3000, k=10, reference_ms=ref_ms, components=want["components"], gpu_equals_reference=bool(same))
    if not same:
        raise SystemExit("the GPU result differs from tests/orientref.py")


def scopes(eng, fn, names, reps):
    eng.profile(1); eng.profile_reset()
    for _ in range(reps):
        fn()
    out = {s: (eng.profile_get(s)[0] / reps, eng.profile_get(s)[1] / reps) for s in names}
    eng.profile(0)
    return out


def run_case(name, args):
    K, N = SIZES[name]
    p, _ = synth.make_view(0, K, N)
    check_subsample(p, name)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], None)
        nrm = eng.estimate_normals(0, 16)["nrm"]
        eng.set_frames([p], [scrambled(nrm, 2)])
        eng.get_structure(0, "scalars")   # waits for the structure builds: nothing else runs while the calls are timed
        n = len(p)
        for k in (10, 16):
            comps = []
            ori = lambda: comps.append(call(eng, eng.lib.mvicp_orient_normals, 0, 0, k, 0.0, 0, None))
            est = lambda: call(eng, eng.lib.mvicp_estimate_normals, 0, k, 0.0, None)
            t_ori, t_est = [], []
            for r in range(args.warm + args.reps):   # alternating
                a, b = once(eng, ori), once(eng, est)
                if r >= args.warm:
                    t_ori.append(a); t_est.append(b)
            s_ori = scopes(eng, ori, KNN_SCOPES + ("orient_round", "orient_finish"), args.reps)
            s_est = scopes(eng, est, KNN_SCOPES + ("normals_pca",), args.reps)
            report(what="orient", case=name, n=n, k=k, reps=args.reps, components=int(comps[-1]),
                   orient_call_median_ms=float(np.median(t_ori)), orient_call_min_ms=float(np.min(t_ori)), orient_call_max_ms=float(np.max(t_ori)),
                   estimate_call_median_ms=float(np.median(t_est)), estimate_call_min_ms=float(np.min(t_est)), estimate_call_max_ms=float(np.max(t_est)),
                   orient_over_estimate_call=float(np.median(t_ori) / np.median(t_est)),
                   search_scopes_ms=sum(s_ori[s][0] for s in KNN_SCOPES), orient_round_ms=s_ori["orient_round"][0],
                   orient_round_launches=s_ori["orient_round"][1], orient_finish_ms=s_ori["orient_finish"][0],
                   estimate_search_scopes_ms=sum(s_est[s][0] for s in KNN_SCOPES), normals_pca_ms=s_est["normals_pca"][0])
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_bench.txt"))
    args = ap.parse_args()
    OUT = open(args.out, "w")
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
