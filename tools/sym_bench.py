"""Micro-benchmark of linearize_sym_kernel next to the point-to-plane linearize_kernel (GPU box).

    python tools/sym_bench.py K N [--pkg DIR] [--out FILE]

synth.make_problem(K, N), one grid search (identity lists: every edge reads p — and, symmetric, n_p — from the shared sorted cloud, two edges
per source).  Symmetric and plane launches ALTERNATE in one process, robust on and off: 2 warm + 7 timed launches each, per launch the
profile scope's own event pair; reported: median (min - max) in us, the library's byte model of the launch, and the fraction of the HBM
peak (8.0 TB/s) it corresponds to.  --pkg DIR takes the package (mvicp/ and its libmvicp_hip.so) from another tree, e.g. a build of the
parent commit: that one has no symmetric kernel, so only its plane kernel is timed, which shows whether that kernel's time moved.
--out appends the lines to FILE."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12   # bytes / s, MI355X
WARM, TIMED = 2, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("K", type=int)
    ap.add_argument("N", type=int)
    ap.add_argument("--pkg", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg) if a.pkg else os.path.join(ROOT, "mv-lm-icp_amd"))
    import mvicp
    from mvicp import lib as L
    from mvicp import synth
    have_sym = hasattr(mvicp.Engine, "linearize_metric")
    pb = synth.make_problem(a.K, a.N)
    print("problem made", flush=True)
    eng = mvicp.Engine(0)
    eng.set_frames(pb["pts"], pb["nor"])
    eng.set_graph(pb["src"], pb["dst"])
    print("clouds and graph on the device", flush=True)
    counts, _ = eng.correspond(pb["init"], pb["fixed"], 0.05, L.NN_GRID)
    print("searched", flush=True)
    eng.profile(True)
    lines = ["sym_bench K=%d N=%d package=%s  correspondences %d (identity lists: %d of %d edges)" % (
        a.K, a.N, a.pkg or "this tree", int(np.sum(counts)), int(np.sum(counts == a.N)), len(counts))]
    for robust in (1, 0):
        t = {"linearize": [], "linearize_sym": []}
        by = {}
        for i in range(WARM + TIMED):
            for scope in ("linearize", "linearize_sym"):
                if scope == "linearize_sym" and not have_sym:
                    continue
                eng.profile_reset()
                if scope == "linearize":
                    eng.linearize(pb["init"], 1, robust)
                else:
                    eng.linearize_metric(pb["init"], L.METRIC_SYMMETRIC, robust)
                ms, n, b = eng.profile_get(scope)
                assert n == 1, (scope, n)
                by[scope] = b
                if i >= WARM:
                    t[scope].append(ms * 1e3)
        for scope, us in t.items():
            if us:
                med = float(np.median(us))
                lines.append("  robust %d  %-14s %8.1f us (%.1f - %.1f)   %7.1f MB / launch   %.2f of the HBM peak" % (
                    robust, scope, med, min(us), max(us), by[scope] / 1e6, by[scope] / (med * 1e-6) / HBM_PEAK))
        if t["linearize_sym"]:
            lines.append("  robust %d  symmetric / plane = %.2f" % (robust, np.median(t["linearize_sym"]) / np.median(t["linearize"])))
    eng.close()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
