#!/usr/bin/env python3
"""Times the voxel-grid reduction (Engine.voxel_grid, csrc/voxel.hip).

  one200k : one synthetic view of 200 000 points, no poses, at the voxel that keeps about 1 point in 8
  one1m   : the same for a view of 1 000 000 points
  fused   : the fused model of 32 x 200 000 points at the synth ground-truth poses, at one200k's voxel

Per case and per value of the option "voxel_permute" (1: the transformed points are laid out in sorted order before the sum, 0: the sum
re-gathers them): WARM untimed calls, then REPS timed ones, each from a drained stream to the call's return (the call waits for its
result; the fetch is not timed); median, min and max in ms.  The result is compared with the numpy statement of the contract
(tests/voxelref.py), whose own time at the same shape is printed as context only.  One JSON line per measurement.

--split runs every case once more in a CHILD process under `rocprofv3 --kernel-trace --stats` (a run of its own) and prints the
kernel time per pass and call from its kernel trace.

    python tools/voxel_bench.py [--cases one200k,one1m,fused] [--reps 7] [--warm 2] [--split] [--no-ref]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvicp  # noqa: E402
from mvicp import synth  # noqa: E402

PASSES = ("cells", "keys", "sort", "runs", "permute", "reduce", "other")


def report(**kw):
    print(json.dumps(kw), flush=True)


def voxel_for_ratio(p, ratio=8.0):
    """Bisection on the host for the voxel edge at which the cloud p keeps about 1 point in `ratio`."""
    lo, hi = 1e-5, float(np.ptp(p, axis=0).max())
    for _ in range(24):
        h = (lo * hi) ** 0.5
        c = np.floor(p / h).astype(np.int64)
        c -= c.min(axis=0)
        d = c.max(axis=0) + 1
        kept = len(np.unique((c[:, 2] * d[1] + c[:, 1]) * d[0] + c[:, 0]))
        if len(p) / kept > ratio:
            hi = h
        else:
            lo = h
    return (lo * hi) ** 0.5


def load_case(name):
    """-> (pts list, nor list, poses or None, voxel)"""
    if name == "fused":
        K, N = 32, 200_000
        views = [synth.make_view(k, K, N) for k in range(K)]
        voxel = voxel_for_ratio(views[0][0])
        return [v[0] for v in views], [v[1] for v in views], synth.make_poses(K)["gt"], voxel
    K, N = {"one200k": (32, 200_000), "one1m": (64, 1_000_000)}[name]
    p, n = synth.make_view(0, K, N)
    return [p], [n], None, voxel_for_ratio(p)


def timed(eng, fn, warm, reps):
    ms = []
    for r in range(warm + reps):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if r >= warm:
            ms.append(1e3 * (t1 - t0))
    ms = np.array(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps}


def grid_only(eng, voxel, P):
    """mvicp_voxel_grid alone (returns when the result is complete on the device)."""
    import ctypes as C
    st = eng.lib.mvicp_voxel_grid(eng.h, 0, None, None if P is None else P.ctypes.data_as(C.POINTER(C.c_double)), float(voxel), None)
    if st < 0:
        raise SystemExit(eng.lib.mvicp_last_error().decode())
    return st


def run_case(name, args):
    pts, nor, poses, voxel = load_case(name)
    P = None if poses is None else mvicp.lib.poses_to_c(poses)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pts, nor)
        eng.get_structure(0, "scalars")   # waits for the structure builds of the upload: nothing else runs while the calls are timed
        n_in = sum(len(p) for p in pts)
        got = {}
        for permute in (1, 0):
            eng.set_option("voxel_permute", permute)
            t = timed(eng, lambda: grid_only(eng, voxel, P), args.warm, args.reps)
            got[permute] = eng.voxel_grid(voxel, None, poses)
            report(what="voxel_grid", case=name, frames=len(pts), points=n_in, voxel=voxel, voxels=len(got[permute]["cnt"]),
                   points_per_voxel=n_in / len(got[permute]["cnt"]), voxel_permute=permute, **t)
        eng.set_option("voxel_permute", 1)
        if not args.no_ref:
            import voxelref
            t0 = time.perf_counter()
            want = voxelref.voxel_grid(pts, nor, voxel, None, poses)
            ref_ms = 1e3 * (time.perf_counter() - t0)
            same = all(voxelref.same(g, want) for g in got.values())
            report(what="numpy_reference", case=name, points=n_in, ms=ref_ms, gpu_equals_reference=same)
            if not same:
                raise SystemExit("the GPU result differs from tests/voxelref.py")
    finally:
        eng.close()


def pass_of(kernel):
    k = kernel.lower()
    for key, name in (("vox_cell", "cells"), ("vox_key", "keys"), ("vox_head", "runs"), ("vox_start", "runs"), ("vox_permute", "permute"), ("vox_reduce", "reduce"),
                      ("sort", "sort"), ("onesweep", "sort"), ("histogram", "sort"), ("scan", "runs")):
        if key in k:
            return name
    return "other"


def split(name, args):
    """The case's calls in a child process under rocprofv3; kernel time per pass and call, from the first to the last voxel kernel."""
    calls = args.warm + args.reps
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "v", "--",
               sys.executable, os.path.abspath(__file__), "--cases", name, "--reps", str(args.reps), "--warm", str(args.warm), "--no-ref", "--child", str(args.child_permute)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 left no kernel trace")
        rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    vox = [i for i, r in enumerate(rows) if "vox_" in r["Kernel_Name"]]
    rows = rows[vox[0]:vox[-1] + 1]
    n_calls = sum(1 for r in rows if "vox_cell" in r["Kernel_Name"])
    assert n_calls == calls + 1, (n_calls, calls)     # (+ the one call whose result is fetched)
    us = dict.fromkeys(PASSES, 0.0)
    for r in rows:
        us[pass_of(r["Kernel_Name"])] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    per_call = {k: v / n_calls / 1e3 for k, v in us.items()}
    report(what="split_ms_per_call", case=name, voxel_permute=args.child_permute, calls=n_calls, kernels_ms=sum(per_call.values()), **per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="one200k,one1m,fused")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--no-ref", dest="no_ref", action="store_true")
    ap.add_argument("--child", type=int, default=-1, help=argparse.SUPPRESS)   # the profiled child: this value of voxel_permute only
    args = ap.parse_args()
    if args.child >= 0:
        name = args.cases
        pts, nor, poses, voxel = load_case(name)
        P = None if poses is None else mvicp.lib.poses_to_c(poses)
        eng = mvicp.Engine(0)
        eng.set_frames(pts, nor)
        eng.get_structure(0, "scalars")
        eng.set_option("voxel_permute", args.child)
        for _ in range(args.warm + args.reps + 1):
            grid_only(eng, voxel, P)
        eng.close()
        return
    for name in args.cases.split(","):
        run_case(name, args)
        if args.split:
            for permute in (1, 0):
                args.child_permute = permute
                split(name, args)


if __name__ == "__main__":
    main()
