#!/usr/bin/env python3
"""Times the ISS keypoints (Engine.iss_keypoints, csrc/iss.hip) and what they buy the clouds-alone initialisation.

  keypoints   one `synth` view of 200 000 and one of 1 000 000 points; the salient radius is the one that holds about 30 and about 100
              neighbours (the median distance to the 30th neighbour of 2 000 sampled points; the second is that times sqrt(100 / 30): the
              cloud is a surface), the suppression radius 0.3 of it.  WARM untimed and REPS timed calls with the profile on: the scopes
              iss_moments, iss_nms, iss_compact, and the wall time from a drained stream to the return of the call.
  floor       in the same session, the knn_count scope of an all-mode self search (mvicp_knn_search, k = 0) at the same radius: the same
              traversal without the moments.  iss_moments / knn_count says what the moments and the eigenvalues cost on top of it.
  matching    K = 8 `synth` views reduced by mvicp_voxel_grid to about 5 000 points, FPFH at 5 voxel edges: Engine.coarse_pairs over all
              i < j edges on all points against on the keypoints (salient radius = the FPFH radius, suppression 0.3 of it), both sides.

No ratio is fixed in advance; one JSON line per measurement, on stdout and in --out.

    python tools/iss_bench.py [--sizes 200000,1000000] [--reps 7] [--warm 2] [--out profiles/iss_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvicp  # noqa: E402
from mvicp import synth  # noqa: E402

import torch  # noqa: E402

from coarse_bench import reduced_views  # noqa: E402

SCOPES = ("iss_moments", "iss_nms", "iss_compact")
H, EDGE_SIM = 10000, 0.9
OUT = None


def report(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()


def timed(eng, fn, warm, reps):
    ms = []
    for r in range(warm + reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        if r >= warm:
            ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def keypoint_leg(eng, n, args):
    pts, nor = synth.make_view(0, 8, n)
    eng.set_frames([pts], [nor])
    rng = np.random.Generator(np.random.PCG64(1))
    sample = np.ascontiguousarray(pts[rng.choice(len(pts), size=2000, replace=False)])
    r30 = float(np.median(np.sqrt(eng.knn_search(0, sample, 31, 0.0)["d2"][:, 30])))
    for want, radius in ((30, r30), (100, r30 * float(np.sqrt(100.0 / 30.0)))):
        iss = lambda: eng.lib.mvicp_iss_keypoints(eng.h, 0, radius, 0.3 * radius, 0.975, 0.975, 5)
        knn = lambda: eng.lib.mvicp_knn_search(eng.h, 0, None, 0, 0, radius)
        k = iss()
        if k < 0:
            raise SystemExit("mvicp_iss_keypoints failed: %r" % eng.lib.mvicp_last_error())
        cnt = eng.iss_keypoints(0, radius, 0.3 * radius)["cnt_salient"]
        eng.profile(1); eng.profile_reset()
        wall = timed(eng, iss, args.warm, args.reps)
        calls = args.warm + args.reps
        sp = {s: eng.profile_get(s)[0] / calls for s in SCOPES}
        eng.profile_reset()
        total = knn()
        if total < 0:
            raise SystemExit("mvicp_knn_search failed: %r" % eng.lib.mvicp_last_error())
        for _ in range(calls - 1):
            knn()
        floor = eng.profile_get("knn_count")[0] / calls
        eng.profile(0)
        report(what="keypoints", points=len(pts), neighbours_wanted=want, radius=radius, neighbours_median=float(np.median(cnt)), neighbours_max=int(cnt.max()),
               keypoints=int(k), wall=wall, scope_ms=sp, knn_count_ms=floor, moments_over_knn_count=sp["iss_moments"] / floor if floor > 0 else None,
               calls_averaged=calls)


def matching_leg(eng, args, K=8, target=5000):
    clouds, normals, voxel = reduced_views(eng, K, target)
    eng.set_frames(clouds, normals)
    radius, tau = 5.0 * voxel, 2.0 * voxel
    descs = [eng.fpfh(i, radius, 64, device=True)["desc"] for i in range(K)]
    kp = [eng.iss_keypoints(i, radius, 0.3 * radius)["idx"] for i in range(K)]
    dev = torch.device("cuda", eng.device)
    edges = [(i, j) for i in range(K) for j in range(i + 1, K)]
    src, dst = [e[0] for e in edges], [e[1] for e in edges]
    out = {}
    for name, rows in (("all_points", [np.arange(len(c)) for c in clouds]), ("keypoints", kp)):
        desc = torch.cat([d.index_select(0, torch.from_numpy(ix.astype(np.int64)).to(dev)) for d, ix in zip(descs, rows)], 0)
        xyz = torch.from_numpy(np.ascontiguousarray(np.concatenate([c[ix] for c, ix in zip(clouds, rows)]))).to(dev)
        torch.cuda.synchronize(dev)
        offsets = np.concatenate([[0], np.cumsum([len(ix) for ix in rows])]).astype(np.int64)
        call = lambda: eng.coarse_pairs(desc, xyz, offsets, src, dst, 0, hypotheses=H, tau=tau, edge_sim=EDGE_SIM)
        res = call()
        out[name] = dict(timed(eng, call, args.warm, args.reps), rows=[int(len(ix)) for ix in rows], inliers=[int(v) for v in res["count"]])
    report(what="matching", views=K, edges=len(edges), hypotheses=H, voxel=voxel, all_points=out["all_points"], keypoints=out["keypoints"],
           all_over_keypoints=out["all_points"]["median_ms"] / out["keypoints"]["median_ms"])


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iss_bench.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    OUT = open(args.out, "w")
    eng = mvicp.Engine(0)
    try:
        for n in (int(x) for x in args.sizes.split(",")):
            keypoint_leg(eng, n, args)
        matching_leg(eng, args)
    finally:
        eng.close()
    OUT.close()


if __name__ == "__main__":
    main()
