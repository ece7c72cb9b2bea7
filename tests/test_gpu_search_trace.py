"""The same launches in the same rounds: three scripted registrations (tests/regime_seq.py, seeds 0 and 1 and the extended script of seed
100, on a 5-frame problem of a few hundred points per frame) are replayed with profiling on, and after every round the NN kernel
instantiation (mvicp_last_nn_launch), the launch counts of the profiled scopes, the counts and the weight bits must equal
tests/golden/search_launch_trace.json — recorded by tools/record_search_trace.py on the commit named in that file, before the search policy
moved into csrc/search_plan.h.  What the searches ANSWER is held to fresh contexts elsewhere (tests/test_gpu_parity.py); this file holds
HOW: which kernel, which launches skipped.  The CPU test checks that the recording went through every regime."""
import json
import os

import pytest

import search_trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_launch_trace.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recorded_trace_covers_every_regime():
    doc = golden()
    assert doc["recorded_by"] == "tools/record_search_trace.py" and len(doc["commit"]) == 40
    assert doc["scopes"] == search_trace.SCOPES and doc["mark"] == search_trace.MARK
    assert (doc["frames"], doc["points"]) == (search_trace.FRAMES, search_trace.POINTS)
    assert [(t["seed"], t["extended"]) for t in doc["traces"]] == search_trace.CASES
    seen = set()
    for t in doc["traces"]:
        assert len(t["rounds"]) == 14
        seen |= search_trace.regimes(t["rounds"])
    assert seen >= search_trace.REQUIRED, search_trace.REQUIRED - seen


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(search_trace.CASES)))
def test_a_scripted_registration_makes_the_recorded_launches(case):
    import mvicp
    seed, extended = search_trace.CASES[case]
    want = golden()["traces"][case]["rounds"]
    eng = mvicp.Engine(0)
    try:
        got = search_trace.record(eng, seed, extended)
    finally:
        eng.close()
    for r, (g, w) in enumerate(zip(got, want)):
        print(r, g["kind"], g["nn"], g["launches"], g["mark"])
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (seed, r, {k: (g[k], w[k]) for k in w if g[k] != w[k]})
