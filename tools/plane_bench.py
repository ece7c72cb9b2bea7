#!/usr/bin/env python3
"""Times the plane stage (Engine.segment_plane, csrc/plane.hip) next to what a user would write on the same device.

  one200k : one synthetic view of 200 000 points (the bench surface) with a planted plane: 30 % more points on a tilted support
            plane under it, sigma 1 mm, shuffled in
  one1m   : the same at 1 000 000 points

Per case and H in {256, 1024, 4096}, tau = 4 mm, seed 0, refine on.  First the result is compared with the numpy statement of the
contract (tests/planeref.py): the whole record, counts and flags where n H <= 3e8 pairs, and on a 20 000-point subsample of the cloud at
the same H for every case (the reference scores every pair in numpy; the larger cases would take minutes of host time).  Then, after
WARM untimed rounds, REPS rounds that ALTERNATE two calls, each timed from a drained stream to the call's return:
  plane     mvicp_segment_plane(H, tau, refine) -- every pass, both host waits; no fetch is timed
  torch     the yardstick, not the code under test: ((P - a) @ M^T).abs() <= tau summed over the points in torch fp64, over the SAME
            accepted hypotheses (a, M uploaded before; P @ M^T - (a . m) in chunks of 32 768 points so that the n x H matrix fits), then
            torch.cuda.synchronize().  It scores only: no sampling, no winner, no refit, no flags.
Medians, minima and maxima in ms, the ratio of the medians, the per-scope kernel times of the library call from its own profile scopes
(HIP events on its stream) over further calls, and the scoring pass's fraction of the fp64 vector peak by its 9-operation model
(9 n A operations for A accepted hypotheses over the plane_score scope; peak 78.6e12 flop/s = 39.3e12 fp64 vector operations per second
counting a fused multiply-add as two, the data sheet's figure -- the kernel issues no fma, so this fraction cannot exceed one half).
mvicp_plane_select is timed the same way.  One JSON line per measurement, to stdout and to --out (default profiles/plane_bench.txt).
No time is asserted.

    python tools/plane_bench.py [--cases one200k,one1m] [--hs 256,1024,4096] [--reps 7] [--warm 2] [--out FILE]
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
import planeref  # noqa: E402
from mvicp import synth  # noqa: E402

SCOPES = ("plane_hyp", "plane_score", "plane_pick", "plane_flags", "plane_moments", "plane_compact")
SIZES = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}
TAU, SEED = 0.004, 0
FULL_CHECK_PAIRS = 3e8
PEAK_FP64_OPS = 78.6e12
CHUNK = 32768
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


def stats(ms):
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": len(ms)}


def make_cloud(K, N):
    """The bench surface with a planted plane -> (points, normals), N points in all."""
    n_plane = (3 * N) // 13           # 30 % of the surface's share
    p, nr = synth.make_view(0, K, N - n_plane)
    rng = np.random.Generator(np.random.PCG64(77))
    nv = np.array([0.05, -0.08, 1.0]); nv /= np.linalg.norm(nv)
    e1 = np.cross(nv, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nv, e1)
    ext = 0.75 * float((p.max(0) - p.min(0))[:2].max())
    uv = rng.uniform(-ext, ext, size=(n_plane, 2))
    plane = p.mean(0) - 0.12 * nv + uv[:, :1] * e1 + uv[:, 1:] * e2 + rng.normal(0.0, 0.001, size=(n_plane, 1)) * nv
    q, qn = np.vstack([p, plane]), np.vstack([nr, np.tile(nv, (n_plane, 1))])
    perm = rng.permutation(len(q))
    return np.ascontiguousarray(q[perm]), np.ascontiguousarray(qn[perm])


def check(eng_factory, p, nr, H, name):
    """The library against tests/planeref.py: the full cloud when it is small enough, and always a 20 000-point subsample."""
    idx = np.linspace(0, len(p) - 1, 20000).astype(np.int64)
    todo = [("subsample", np.ascontiguousarray(p[idx]), np.ascontiguousarray(nr[idx]))]
    if len(p) * H <= FULL_CHECK_PAIRS:
        todo.append(("full", p, nr))
    for what, q, qn in todo:
        eng = eng_factory()
        try:
            eng.set_frames([q], [qn])
            t0 = time.perf_counter()
            want = planeref.segment(q, qn, TAU, H, SEED)
            ref_ms = 1e3 * (time.perf_counter() - t0)
            got = eng.segment_plane(0, TAU, H, SEED)
            same = planeref.same(got, want) and all(planeref.same_kept(eng.plane_select(k), planeref.select(q, qn, want, k)) for k in (True, False))
        finally:
            eng.close()
        report(what="numpy_reference", case=name, H=H, points=len(q), cloud=what, ms=ref_ms, accepted=want["accepted"], count=want["count"],
               count_refined=want["count_refined"], gpu_equals_reference=same)
        if not same:
            raise SystemExit("the GPU result differs from tests/planeref.py")


def run_case(name, args):
    import torch
    K, N = SIZES[name]
    p, nr = make_cloud(K, N)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames([p], [nr])
        eng.get_structure(0, "scalars")   # waits for the structure build: nothing else runs while the calls are timed
        lib, h = eng.lib, eng.h
        P = torch.from_numpy(p).to("cuda:0")
        for H in args.hs:
            check(lambda: mvicp.Engine(0), p, nr, H, name)
            ok, a, m = planeref.hypotheses(p, H, SEED)
            A, M = torch.from_numpy(np.ascontiguousarray(a[ok])).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(m[ok])).to("cuda:0")
            R = mvicp.lib.PlaneResult()

            def plane():
                return must(eng, lib.mvicp_segment_plane(h, 0, H, SEED, TAU, None, 0.0, 1, C.byref(R)))

            def yard():
                off = (A * M).sum(1)
                cnt = torch.zeros(len(A), dtype=torch.int64, device="cuda:0")
                for lo in range(0, len(P), CHUNK):
                    cnt += ((P[lo:lo + CHUNK] @ M.T - off).abs() <= TAU).sum(0)
                torch.cuda.synchronize()
                return cnt

            calls = {"plane": plane, "torch": yard}
            ms = {key: [] for key in calls}
            out = {}
            for r in range(args.warm + args.reps):
                for key, fn in calls.items():
                    eng.sync(); torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out[key] = fn()
                    t1 = time.perf_counter()
                    if r >= args.warm:
                        ms[key].append(1e3 * (t1 - t0))
            t = {key: stats(v) for key, v in ms.items()}
            counts = eng.segment_plane(0, TAU, H, SEED)["counts"]
            ycnt = out["torch"].cpu().numpy()
            differ = int((counts[ok] != ycnt).sum())   # (the yardstick rounds differently: a point at the edge of tau may fall the other way)
            report(what="plane", case=name, points=N, H=H, tau=TAU, accepted=int(R.accepted), count=int(R.count), count_refined=int(R.count_refined), **t["plane"])
            report(what="yardstick_torch_fp64", case=name, H=H, accepted=int(ok.sum()), counts_that_differ_from_the_contract=differ,
                   largest_count_difference=int(np.abs(counts[ok].astype(np.int64) - ycnt).max()) if ok.any() else 0, **t["torch"])
            report(what="ratio_of_medians", case=name, H=H, plane_over_torch=t["plane"]["median_ms"] / t["torch"]["median_ms"])
            sel = []
            for r in range(args.warm + args.reps):
                eng.sync()
                t0 = time.perf_counter()
                kept = must(eng, lib.mvicp_plane_select(h, 0))
                if r >= args.warm:
                    sel.append(1e3 * (time.perf_counter() - t0))
            report(what="plane_select_rest", case=name, H=H, kept=int(kept), **stats(sel))
            eng.profile(1); eng.profile_reset()
            for _ in range(args.reps):
                plane()
                must(eng, lib.mvicp_plane_select(h, 0))
            split = {s: eng.profile_get(s)[0] / args.reps for s in SCOPES}
            eng.profile(0)
            ops = 9.0 * N * int(R.accepted)
            report(what="split_ms_per_call", case=name, H=H, kernels_ms=sum(split.values()), score_model_ops=ops,
                   score_fraction_of_fp64_vector_peak=(ops / (split["plane_score"] * 1e-3)) / PEAK_FP64_OPS if split["plane_score"] > 0 else None, **split)
    finally:
        eng.close()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m")
    ap.add_argument("--hs", default="256,1024,4096")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_bench.txt"))
    args = ap.parse_args()
    args.hs = [int(v) for v in args.hs.split(",")]
    OUT = open(args.out, "w")
    OUT.write("# tools/plane_bench.py on one MI355X (gfx950): the plane stage (mvicp_segment_plane, DESIGN.md section 3.19), tau %g, seed %d, refine on\n"
              "# %d warm + %d timed rounds that alternate plane (the whole call, both host waits) / torch (the yardstick: P @ M^T - a.m, abs, <= tau, sum,\n"
              "# fp64, the same accepted hypotheses, chunks of %d points), wall ms from a drained stream to the call's return; split_ms_per_call: the\n"
              "# library's profile scopes (HIP events) over %d further calls of mvicp_segment_plane + mvicp_plane_select; numpy_reference: tests/planeref.py\n"
              "# on what the GPU result is compared with first (the full cloud up to %g pairs, a 20 000-point subsample always; context only).\n"
              % (TAU, SEED, args.warm, args.reps, CHUNK, args.reps, FULL_CHECK_PAIRS))
    for name in args.cases.split(","):
        run_case(name, args)
    OUT.close()


if __name__ == "__main__":
    main()
