#!/usr/bin/env python3
"""Records tests/golden/search_launch_trace.json: which NN kernel and how many launches per profiled scope every round of three scripted
registrations makes (tests/search_trace.py).  Run it on the commit whose behaviour is to be kept, on the GPU the suite runs on:

    python tools/record_search_trace.py --commit $(git rev-parse HEAD) [--out FILE] [--points N] [--cases 0,1,100x]

tests/test_gpu_search_trace.py then holds later commits to the recorded launches.  A case is a seed of tests/regime_seq.py, "x" = extended."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mv-lm-icp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mvicp  # noqa: E402
import search_trace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit the trace is recorded on")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "search_launch_trace.json"))
    ap.add_argument("--points", type=int, default=search_trace.POINTS)
    ap.add_argument("--cases", default=",".join(f"{s}{'x' if x else ''}" for s, x in search_trace.CASES))
    args = ap.parse_args()
    cases = [(int(t.rstrip("x")), t.endswith("x")) for t in args.cases.split(",")]
    doc = {"recorded_by": "tools/record_search_trace.py", "commit": args.commit, "frames": search_trace.FRAMES, "points": args.points,
           "scopes": search_trace.SCOPES, "mark": search_trace.MARK, "traces": []}
    seen = set()
    for seed, extended in cases:
        eng = mvicp.Engine(0)
        try:
            rounds = search_trace.record(eng, seed, extended, args.points)
        finally:
            eng.close()
        got = search_trace.regimes(rounds)
        seen |= got
        print(f"seed {seed}{' extended' if extended else ''}: {sorted(got)}")
        for r in rounds:
            print("   %-8s %-22s %s mark %d" % (r["kind"], r["nn"], r["launches"], r["mark"]))
        doc["traces"].append({"seed": seed, "extended": extended, "rounds": rounds})
    missing = search_trace.REQUIRED - seen
    print("regimes missing over all cases:", sorted(missing) if missing else "none")
    with open(args.out, "w") as f:
        f.write("{\n")
        for k, v in doc.items():
            if k != "traces":
                f.write(f" {json.dumps(k)}: {json.dumps(v)},\n")
        f.write(' "traces": [\n')
        for i, t in enumerate(doc["traces"]):
            f.write(f'  {{"seed": {t["seed"]}, "extended": {json.dumps(t["extended"])}, "rounds": [\n')
            f.write(",\n".join("   " + json.dumps(r) for r in t["rounds"]))
            f.write("\n  ]}" + ("," if i + 1 < len(doc["traces"]) else "") + "\n")
        f.write(" ]\n}\n")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
