#!/usr/bin/env python3
"""Times the batched coarse poses (Engine.coarse_pairs, csrc/coarse.hip) against the loop of single-pair calls it replaces.

  inputs      K = 8 and 32 `synth` views, each reduced by mvicp_voxel_grid to about 2 000 and about 5 000 points (the voxel edge is found by
              bisection on view 0), FPFH on the device (radius 5 voxel edges, max_nn 64), descriptors resident on the device; all i < j
              edges, H = 10 000, tau = 2 voxel edges, edge_sim 0.9, mutual matches, no ratio test, seeds[e] = e.
  batched     ONE Engine.coarse_pairs over the concatenated device descriptors and points.
  loop        NOT new code, the yardstick: per edge Engine.feature_match (device descriptors) -> mvicp.match_pairs -> the gather on the host
              -> Engine.consensus, as mvicp.coarse_align chains them.
  protocol    the two legs alternate in one process: WARM untimed and REPS timed repetitions of each, from a drained stream to the return of
              the last call; medians, with min and max.  Then the library's profile scopes of the batched call over REPS further calls.
  equality    before timing, every edge's record and fetched pairs / flags of the batched call are compared with the loop's, byte for byte;
              a difference ends the run.
  rates       coarse_match against the instruction-count bound of the contract, m n dim 3 fp64 operations per table (subtract, multiply,
              add: no fma) summed over the distinct tables -- the early exit skips operations the bound counts, so the figure is an
              effective rate -- and as a fraction of 39.3e12/s, the device's published vector fp64 rate (78.6 Tflop/s) with an fma counted
              once; coarse_score against accepted x pairs x 26 operations.

No speed-up is fixed in advance; one JSON line per measurement, on stdout and in --out.

    python tools/coarse_bench.py [--views 8,32] [--points 2000,5000] [--reps 7] [--warm 2] [--out profiles/coarse_bench.txt]
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
from mvicp import synth  # noqa: E402

import torch  # noqa: E402

SCOPES = ("coarse_match", "coarse_merge", "coarse_rule", "coarse_hyp", "coarse_score", "coarse_pick")
PEAK_OPS = 39.3e12   # vector fp64 operations per second with an fma counted once (published: 78.6 Tflop/s counting it twice)
SCORE_OPS = 26       # fp64 operations of one (hypothesis, pair) score: R p (15), + t (3), - q (3), dot (5)
H, EDGE_SIM = 10000, 0.9
OUT = None


def report(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def reduced_views(eng, K, target):
    """K synth views, each reduced to one point per voxel; the edge that takes view 0 to about `target` points -> (xyz [K], nrm [K], voxel)"""
    views = [synth.make_view(i, K, 4 * target) for i in range(K)]
    eng.set_frames([v[0] for v in views], [v[1] for v in views])
    lo, hi = 1e-4, 1.0
    for _ in range(30):
        mid = math_sqrt(lo * hi)
        n = len(eng.voxel_grid(mid, [0])["cnt"])
        if n > target:
            lo = mid
        else:
            hi = mid
        if abs(n - target) <= target // 50:
            break
    levels = [eng.voxel_grid(mid, [i]) for i in range(K)]
    return [lv["xyz"] for lv in levels], [lv["nrm"] for lv in levels], mid


def math_sqrt(x):
    return float(np.sqrt(x))


def loop_leg(eng, descs, clouds, edges, tau):
    out = []
    for e, (i, j) in enumerate(edges):
        mt = eng.feature_match(descs[i], descs[j])
        pairs = mvicp.match_pairs(mt["fwd_idx"], mt["fwd_d2"], mt["bwd_idx"], True, 1.0)
        rec = {"pairs": len(pairs), "best": -1, "count": 0, "accepted": 0, "pose": np.eye(4), "list": pairs, "flags": np.zeros(len(pairs), dtype=np.uint8)}
        if len(pairs) >= 3:
            P, Q = np.ascontiguousarray(clouds[i][pairs[:, 0]]), np.ascontiguousarray(clouds[j][pairs[:, 1]])
            cons = eng.consensus(P, Q, H, e, tau, EDGE_SIM)
            rec.update(best=cons["best"], count=cons["count"], accepted=cons["accepted"], pose=cons["pose"], flags=cons["flags"])
        out.append(rec)
    return out


def run(eng, K, target, args):
    clouds, normals, voxel = reduced_views(eng, K, target)
    eng.set_frames(clouds, normals)
    radius, tau = 5.0 * voxel, 2.0 * voxel
    descs = [eng.fpfh(i, radius, 64, device=True)["desc"] for i in range(K)]
    dev = torch.device("cuda", eng.device)
    desc = torch.cat(descs, 0)
    xyz = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds))).to(dev)
    torch.cuda.synchronize(dev)
    sizes = [len(c) for c in clouds]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    edges = [(i, j) for i in range(K) for j in range(i + 1, K)]
    src, dst = [e[0] for e in edges], [e[1] for e in edges]
    batched = lambda: eng.coarse_pairs(desc, xyz, offsets, src, dst, 0, hypotheses=H, tau=tau, edge_sim=EDGE_SIM)
    loop = lambda: loop_leg(eng, descs, clouds, edges, tau)
    # equality first, at the size that is timed
    res, want = batched(), loop()
    for e, w in enumerate(want):
        pr, fl = eng.coarse_pairs_fetch(e)
        same = (all(int(res[k][e]) == int(w[k]) for k in ("pairs", "best", "count", "accepted")) and res["pose"][e].tobytes() == w["pose"].tobytes() and
                pr.tobytes() == w["list"].tobytes() and fl.tobytes() == w["flags"].tobytes())
        if not same:
            raise SystemExit("edge %d %r: the batched call differs from the loop of single calls" % (e, edges[e]))
    usable = int(sum(1 for w in want if w["count"] >= 20))
    report(what="equality", views=K, points=sizes, voxel=voxel, edges=len(edges), batched_equals_loop=True, edges_with_20_inliers=usable,
           pairs_median=float(np.median([w["pairs"] for w in want])), accepted_median=float(np.median([w["accepted"] for w in want])))
    ms = {"batched": [], "loop": []}
    for r in range(args.warm + args.reps):
        for name, fn in (("batched", batched), ("loop", loop)):
            eng.sync()
            t0 = time.perf_counter()
            fn()
            eng.sync()
            t1 = time.perf_counter()
            if r >= args.warm:
                ms[name].append(1e3 * (t1 - t0))
    stat = {name: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for name, v in ms.items()}
    report(what="legs", views=K, points_median=int(np.median(sizes)), edges=len(edges), hypotheses=H, reps=args.reps, warm=args.warm, batched=stat["batched"],
           loop_of_single_calls=stat["loop"], loop_over_batched=stat["loop"]["median_ms"] / stat["batched"]["median_ms"])
    eng.profile(1); eng.profile_reset()
    for _ in range(args.reps):
        batched()
    sp = {s: eng.profile_get(s)[0] / args.reps for s in SCOPES}
    eng.profile(0)
    match_ops = 2.0 * sum(3.0 * 33 * sizes[i] * sizes[j] for i, j in edges)   # both tables of every edge; each distinct table once
    score_ops = float(sum(float(w["accepted"]) * w["pairs"] * SCORE_OPS for w in want))
    report(what="scopes", views=K, points_median=int(np.median(sizes)), edges=len(edges), scope_ms=sp, match_bound_ops=match_ops,
           match_effective_Gops=match_ops / (sp["coarse_match"] * 1e-3) / 1e9, match_fraction_of_published_rate=match_ops / (sp["coarse_match"] * 1e-3) / PEAK_OPS,
           score_bound_ops=score_ops, score_Gops=score_ops / (sp["coarse_score"] * 1e-3) / 1e9 if sp["coarse_score"] > 0 else None,
           score_fraction_of_published_rate=score_ops / (sp["coarse_score"] * 1e-3) / PEAK_OPS if sp["coarse_score"] > 0 else None,
           scopes_sum_ms=float(sum(sp.values())))


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="8,32")
    ap.add_argument("--points", default="2000,5000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT = open(args.out, "w")
    eng = mvicp.Engine(0)
    try:
        for K in (int(x) for x in args.views.split(",")):
            for target in (int(x) for x in args.points.split(",")):
                run(eng, K, target, args)
    finally:
        eng.close()
    OUT.close()


if __name__ == "__main__":
    main()
