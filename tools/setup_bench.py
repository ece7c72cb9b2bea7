"""Per-cloud structure build on the host (mvicp_set_frame) against the device build (mvicp_set_frame_device), on the cfg4 / cfg5
synthetic problems, both builds alternated in one process.

Prints, per config: the per-cloud build time of both (host wall without the upload; for the device build also its kernels' time by
device events), the set-up wall time (set_frames + set_graph) through both entry points, and a byte comparison of every structure array
of every cloud (`identical: true`).  The last line is one JSON record.

  python tools/setup_bench.py [--cfg cfg4,cfg5] [--reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))

import torch  # noqa: E402
import mvicp  # noqa: E402
from mvicp import lib as L  # noqa: E402
from mvicp import synth  # noqa: E402

CFGS = {"cfg4": (32, 200000), "cfg5": (64, 1000000)}


def per_cloud(pts, nor, tens, tnor, device):
    """One synchronous build per cloud (async_build 0): build_ms of every frame."""
    e = mvicp.Engine(0)
    try:
        e.set_option("async_build", 0)
        e.set_frames([pts[0][:1]] * len(pts))
        out = []
        for i in range(len(pts)):
            if device:
                e.set_frame_device(i, tens[i], tnor[i])
            else:
                e.set_frame(i, pts[i], nor[i])
            out.append(e.get_structure(i, "build_ms").copy())
        return np.array(out)
    finally:
        e.close()


def setup(pb, tens, tnor, device):
    """set_frames + set_graph through one entry point, default options (background builds); returns (seconds, engine)."""
    e = mvicp.Engine(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if device:
        e.set_frames_device(tens, tnor)
    else:
        e.set_frames(pb["pts"], pb["nor"])
    t1 = time.perf_counter()
    e.set_graph(pb["src"], pb["dst"])
    t2 = time.perf_counter()
    return (t1 - t0, t2 - t1), e


def compare(eh, ed, K):
    for f in range(K):
        for name in L.STRUCTURE_NAMES:
            a, b = eh.get_structure(f, name).view(np.uint8), ed.get_structure(f, name).view(np.uint8)
            if a.size != b.size or not np.array_equal(a, b):
                return False, f"frame {f} {name}"
    return True, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg4,cfg5")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    rec = {}
    for cfg in a.cfg.split(","):
        K, N = CFGS[cfg]
        pb = synth.make_problem(K, N)
        tens = [torch.from_numpy(p).to("cuda:0") for p in pb["pts"]]
        tnor = [torch.from_numpy(n).to("cuda:0") for n in pb["nor"]]
        torch.cuda.synchronize()
        r = {"views": K, "points": N}
        for rep in range(a.reps):   # alternated; the last repetition is reported (the first one loads the code objects)
            host = per_cloud(pb["pts"], pb["nor"], tens, tnor, False)
            dev = per_cloud(pb["pts"], pb["nor"], tens, tnor, True)
        r["build_ms_host_median"] = float(np.median(host[:, 0]))
        r["build_ms_device_wall_median"] = float(np.median(dev[:, 0]))
        r["build_ms_device_kernels_median"] = float(np.median(dev[:, 1]))
        r["build_s_host_sum"] = float(host[:, 0].sum() / 1e3)
        r["build_s_device_sum"] = float(dev[:, 0].sum() / 1e3)
        for rep in range(a.reps):
            (hf, hg), eh = setup(pb, tens, tnor, False)
            if rep + 1 < a.reps:
                eh.close()
            (df, dg), ed = setup(pb, tens, tnor, True)
            if rep + 1 < a.reps:
                ed.close()
        r["setup_s_host"] = {"set_frames": hf, "set_graph": hg, "total": hf + hg}
        r["setup_s_device"] = {"set_frames": df, "set_graph": dg, "total": df + dg}
        same, where = compare(eh, ed, K)
        r["identical"] = same
        if where:
            r["first_difference"] = where
        eh.close(); ed.close()
        print(f"{cfg}: per-cloud build host {r['build_ms_host_median']:.1f} ms, device {r['build_ms_device_wall_median']:.1f} ms wall "
              f"({r['build_ms_device_kernels_median']:.1f} ms kernels); set-up host {hf + hg:.3f} s (set_frames {hf:.3f} + set_graph {hg:.3f}), "
              f"device {df + dg:.3f} s (set_frames {df:.3f} + set_graph {dg:.3f}); identical: {str(same).lower()}", flush=True)
        rec[cfg] = r
        del tens, tnor
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
