#!/usr/bin/env python3
"""Times descriptor matching (Engine.feature_match, csrc/match.hip) and the consensus coarse pose (Engine.consensus, csrc/consensus.hip).

  feature_match   dim = 33, m = n = 5 000 / 20 000 / 50 000: the FPFH descriptors (mvicp_fpfh, 30-neighbour radius, max_nn = 64) of two
                  `synth` views, resident on the device and passed as device pointers.  At 5 000 the result is first compared with the
                  numpy statement of the contract (tests/matchref.py).  Per option value match_chunk in --chunks: WARM untimed and REPS
                  timed calls of mvicp_feature_match, from a drained stream to the call's return (finiteness check, both directions,
                  merge), and the library's own profile scopes ("match_fwd", "match_bwd", "match_merge": HIP events on its stream) over
                  further calls.  Reported against the instruction-count bound of the contract: m n dim 3 fp64 operations (subtract,
                  multiply, add: no fma) for one direction, as operations per second of the "match_fwd" scope -- the early exit skips
                  operations the bound counts, so the figure is an effective rate -- and as a fraction of 39.3e12/s, the device's
                  published vector fp64 rate (78.6 Tflop/s) with an fma counted once.
  yardstick       NOT the code under test: the same device's torch.cdist in fp64 followed by topk(2, largest=False) along both axes, which
                  is what a user would otherwise write.  It is inexact (cdist expands |a|^2 + |b|^2 - 2 a.b and takes a square root).
  consensus       c = 1 000 / 10 000 pairs with H = 10 000 / 100 000: points of a `synth` view and their images under a rigid motion, 70 %
                  of the pairs replaced by wrong ones; edge_sim = 0.9, tau = 0.01.  The call, the scopes "cons_hyp", "cons_score",
                  "cons_pick", and the bound of the scoring pass: accepted hypotheses x c x 26 fp64 operations.

No ratio is fixed in advance; one JSON line per measurement, on stdout and in --out.

    python tools/match_bench.py [--sizes 5000,20000,50000] [--chunks 512,1024,2048,4096,8192] [--reps 7] [--warm 2] [--out profiles/match_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvicp  # noqa: E402
import matchref  # noqa: E402
from mvicp import synth  # noqa: E402

import torch  # noqa: E402

MATCH_SCOPES = ("match_fwd", "match_bwd", "match_merge")
CONS_SCOPES = ("cons_hyp", "cons_score", "cons_pick")
PEAK_OPS = 39.3e12   # vector fp64 operations per second with an fma counted once (published: 78.6 Tflop/s counting it twice)
SCORE_OPS = 26       # fp64 operations of one (hypothesis, pair) score: R p (15), + t (3), - q (3), dot (5)
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


def timed(sync, fn, warm, reps):
    ms = []
    for r in range(warm + reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        t1 = time.perf_counter()
        if r >= warm:
            ms.append(1e3 * (t1 - t0))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def scopes(eng, fn, names, reps):
    eng.profile(1); eng.profile_reset()
    for _ in range(reps):
        fn()
    out = {s: eng.profile_get(s)[0] / reps for s in names}
    eng.profile(0)
    return out


def descriptors(eng, n):
    """the FPFH descriptors of two synth views of n points each, as device tensors"""
    views = [synth.make_view(i, 8, n) for i in range(2)]
    eng.set_frames([v[0] for v in views], [v[1] for v in views])
    q = np.ascontiguousarray(views[0][0][np.linspace(0, n - 1, 2000).astype(np.int64)])
    radius = float(np.sqrt(np.median(eng.knn_search(0, q, 31)["d2"][:, 30])))
    return [eng.fpfh(i, radius, 64, device=True)["desc"] for i in range(2)], radius


def run_match(eng, n, args):
    (a, b), radius = descriptors(eng, n)
    m = n
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    if n <= 5000:
        t0 = time.perf_counter()
        want = matchref.feature_match(a.cpu().numpy(), b.cpu().numpy())
        ref_ms = 1e3 * (time.perf_counter() - t0)
        same = matchref.same(eng.feature_match(a, b), want, matchref.MATCH_KEYS)
        report(what="numpy_reference", m=m, n=n, dim=33, reference_ms=ref_ms, gpu_equals_reference=bool(same))
        if not same:
            raise SystemExit("the GPU result differs from tests/matchref.py")
    ops = 3.0 * 33 * m * n
    fn = lambda: call(eng, eng.lib.mvicp_feature_match, pa, m, pb, n, 33)
    for chunk in args.chunks:
        eng.set_option("match_chunk", chunk)
        t = timed(eng.sync, fn, args.warm, args.reps)
        sp = scopes(eng, fn, MATCH_SCOPES, args.reps)
        report(what="feature_match", m=m, n=n, dim=33, radius=radius, match_chunk=chunk, call_median_ms=t["median_ms"], call_min_ms=t["min_ms"],
               call_max_ms=t["max_ms"], reps=args.reps, match_fwd_ms=sp["match_fwd"], match_bwd_ms=sp["match_bwd"], match_merge_ms=sp["match_merge"],
               bound_ops_one_direction=ops, fwd_effective_Gops=ops / (sp["match_fwd"] * 1e-3) / 1e9,
               fwd_fraction_of_published_rate=ops / (sp["match_fwd"] * 1e-3) / PEAK_OPS)
    eng.set_option("match_chunk", 2048)

    def yardstick():
        D = torch.cdist(a, b)
        f = D.topk(min(2, n), dim=1, largest=False)
        g = D.topk(min(2, m), dim=0, largest=False)
        return f, g
    t = timed(torch.cuda.synchronize, yardstick, args.warm, args.reps)
    report(what="yardstick_torch_cdist_topk2", m=m, n=n, dim=33, median_ms=t["median_ms"], min_ms=t["min_ms"], max_ms=t["max_ms"], reps=args.reps,
           note="inexact; not the code under test")


def consensus_pairs(c, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    p, _ = synth.make_view(0, 8, max(c, 2000))
    P = np.ascontiguousarray(p[rng.permutation(len(p))[:c]])
    R = synth.so3_exp(np.array([0.3, -0.5, 0.2])); t = np.array([0.1, 0.05, -0.2])
    Q = P @ R.T + t
    wrong = rng.random(c) < 0.7
    Q[wrong] = Q[rng.permutation(c)][wrong]
    return P, np.ascontiguousarray(Q)


def run_consensus(eng, c, H, args):
    P, Q = consensus_pairs(c, 3)
    dev = torch.device("cuda", eng.device)
    dP, dQ = torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev)
    torch.cuda.synchronize(dev)
    res = mvicp.lib.ConsensusResult()
    fn = lambda: call(eng, eng.lib.mvicp_consensus, C.c_void_p(dP.data_ptr()), C.c_void_p(dQ.data_ptr()), c, H, 12345, 0.01, 0.9, C.byref(res))
    t = timed(eng.sync, fn, args.warm, args.reps)
    sp = scopes(eng, fn, CONS_SCOPES, args.reps)
    ops = float(res.accepted) * c * SCORE_OPS
    report(what="consensus", pairs=c, hypotheses=H, accepted=int(res.accepted), best=int(res.best), inliers=int(res.count), call_median_ms=t["median_ms"],
           call_min_ms=t["min_ms"], call_max_ms=t["max_ms"], reps=args.reps, cons_hyp_ms=sp["cons_hyp"], cons_score_ms=sp["cons_score"],
           cons_pick_ms=sp["cons_pick"], bound_ops_score=ops, score_Gops=ops / (sp["cons_score"] * 1e-3) / 1e9 if sp["cons_score"] > 0 else None,
           score_fraction_of_published_rate=ops / (sp["cons_score"] * 1e-3) / PEAK_OPS if sp["cons_score"] > 0 else None)


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000,20000,50000")
    ap.add_argument("--chunks", default="512,1024,2048,4096,8192")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.txt"))
    args = ap.parse_args()
    args.chunks = [int(x) for x in args.chunks.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT = open(args.out, "w")
    eng = mvicp.Engine(0)
    try:
        for n in (int(x) for x in args.sizes.split(",")):
            run_match(eng, n, args)
        for c in (1000, 10000):
            for H in (10000, 100000):
                run_consensus(eng, c, H, args)
    finally:
        eng.close()
    OUT.close()


if __name__ == "__main__":
    main()
