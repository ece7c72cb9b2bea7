"""Which launches a scripted registration makes, round by round (TEST INFRASTRUCTURE, shared by tools/record_search_trace.py, which records
the golden trace, and tests/test_gpu_search_trace.py, which replays it).

A search's answer is checked against fresh contexts elsewhere (tests/test_gpu_parity.py); the trace pins down HOW the answer was found: the
NN kernel instantiation of every round (mvicp_last_nn_launch) and how many launches each profiled scope made in it.  The policy that decides
them is csrc/search_plan.h."""
import numpy as np

import regime_seq

# (seed of regime_seq.script, extended)
CASES = [(0, False), (1, False), (100, True)]
FRAMES, POINTS = 5, 600
SCOPES = ["nn_brute", "nn_grid", "nn_far", "nn_tie", "compact", "gather", "select", "linearize", "linearize_pair"]
# not a launch: written once per cache-aware tile round that weighs the two tile builds (api.cpp, "auto.eps_over_mu")
MARK = "auto.eps_over_mu"


def problem(seed, points=POINTS):
    from mvicp import synth
    return synth.make_problem(FRAMES, points, cone_deg=100.0 if seed % 2 == 0 else 45.0, pose_seed=800 + seed)


def record(eng, seed, extended, points=POINTS):
    """Replays script (seed, extended) on a fresh engine -> list of per-round dicts: {"kind", "nn", "launches": [per SCOPES], "mark", "counts",
    "weights" (float32 bit patterns)}.  Launch counts are per round (the failed search of a "fail" round included)."""
    pb = problem(seed, points)
    eng.set_frames(pb["pts"], pb["nor"])
    eng.set_graph(pb["src"], pb["dst"])
    eng.profile(True)
    rounds = []
    last = {s: 0 for s in SCOPES + [MARK]}

    def after_round(state):
        now = {s: int(eng.profile_get(s)[1]) for s in SCOPES + [MARK]}
        rounds.append({"kind": state["event"]["kind"], "nn": eng.last_nn_launch(),
                       "launches": [now[s] - last[s] for s in SCOPES], "mark": now[MARK] - last[MARK],
                       "counts": [int(v) for v in state["counts"]],
                       "weights": [int(v) for v in np.asarray(state["weights"], dtype=np.float32).view(np.uint32)]})
        last.update(now)

    regime_seq.run(eng, pb, regime_seq.script(seed, FRAMES, extended=extended), after_round=after_round)
    return rounds


def bounds_build(nn):
    """the BND template argument of a tile launch ("tile<WPE,TOP,BND>", "mfma<WPE,TOP,BND,...>"), None for the other kernels"""
    if not (nn.startswith("tile<") or nn.startswith("mfma<")):
        return None
    return int(nn[nn.index("<") + 1:-1].split(",")[2])


def regimes(rounds):
    """-> the set of search regimes the rounds of one trace went through"""
    got = set()
    i_far, i_tie, i_compact = SCOPES.index("nn_far"), SCOPES.index("nn_tie"), SCOPES.index("compact")
    for r in rounds:
        bnd = bounds_build(r["nn"])
        if bnd == 0:
            got.add("tile")
        elif bnd == 1:
            got.add("cache-aware tile" if r["mark"] else "hand-over")
        elif r["nn"] == "grid" and r["kind"] != "fail":
            if r["launches"][i_compact] == 0 and (r["launches"][i_far] == 0 or r["launches"][i_tie] == 0):
                got.add("grid with skipped launches")
    return got


REQUIRED = {"tile", "hand-over", "cache-aware tile", "grid with skipped launches"}
