"""Micro-benchmark of linearize_gicp_kernel next to linearize_sym_kernel (GPU box).

    python tools/gicp_bench.py [--shapes K:N,K:N] [--epsilon E] [--out FILE]

Per shape (default: cfg4's, 32 frames of 200 000 points, and a smaller one, 8 of 50 000): synth.make_problem(K, N), one grid search (identity
lists: every edge reads p and n_p from the shared sorted cloud), then plane-to-plane and symmetric launches ALTERNATE on the same lists in one
process, robust on and off: 2 warm + 7 timed launches each, per launch the profile scope's own event pair.  Reported: median (min - max) in
us, the library's byte model of the launch, the fraction of the HBM peak (8.0 TB/s) it corresponds to, and the figure this tool exists for:
the plane-to-plane launch against the symmetric launch measured in the same run.  No time is asserted.  The lines are written to
profiles/gicp_bench.txt (--out FILE: elsewhere)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12   # bytes / s, MI355X
WARM, TIMED = 2, 7


def bench_shape(K, N, eps):
    import mvicp
    from mvicp import lib as L
    from mvicp import synth
    pb = synth.make_problem(K, N)
    print("problem made", flush=True)
    eng = mvicp.Engine(0)
    try:
        eng.set_frames(pb["pts"], pb["nor"])
        eng.set_graph(pb["src"], pb["dst"])
        counts, _ = eng.correspond(pb["init"], pb["fixed"], 0.05, L.NN_GRID)
        print("searched", flush=True)
        eng.profile(True)
        lines = ["gicp_bench K=%d N=%d epsilon=%g  correspondences %d (identity lists: %d of %d edges)" % (
            K, N, eps, int(np.sum(counts)), int(np.sum(counts == N)), len(counts))]
        for robust in (1, 0):
            t = {"linearize_sym": [], "linearize_gicp": []}
            by = {}
            for i in range(WARM + TIMED):
                for scope in t:
                    eng.profile_reset()
                    if scope == "linearize_sym":
                        eng.linearize_metric(pb["init"], L.METRIC_SYMMETRIC, robust)
                    else:
                        eng.linearize_gicp(pb["init"], eps, robust)
                    ms, n, b = eng.profile_get(scope)
                    assert n == 1, (scope, n)
                    by[scope] = b
                    if i >= WARM:
                        t[scope].append(ms * 1e3)
            for scope, us in t.items():
                med = float(np.median(us))
                lines.append("  robust %d  %-14s %8.1f us (%.1f - %.1f)   %7.1f MB / launch   %.2f of the HBM peak" % (
                    robust, scope, med, min(us), max(us), by[scope] / 1e6, by[scope] / (med * 1e-6) / HBM_PEAK))
            lines.append("  robust %d  gicp / symmetric = %.2f" % (robust, np.median(t["linearize_gicp"]) / np.median(t["linearize_sym"])))
        return lines
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32:200000,8:50000")
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_bench.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
    lines = []
    for shape in a.shapes.split(","):
        K, N = (int(x) for x in shape.split(":"))
        lines += bench_shape(K, N, a.epsilon)
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
