"""The scripts that the sharded regime tests replay (tests/regime_seq.py) are pure functions of their arguments, and the tests' coverage is what
those scripts happen to hold: a change to the generator must not move them.  Digests recorded before regime_seq.script learnt `metrics`."""
import hashlib
import json

import pytest

import regime_seq

DIGESTS = {
    0: "76a6a35895ae0771feb0360a1c7264a10313237467d9fc2c8740605b119bd6c7",
    1: "d9ad2379ac27658c17143922f3629bef44b6d8d8b191fa6e2c434b6ba716fe57",
    2: "92c329e1f1085c156314ee8be295b9483a4f7db2329d08ba5d1b78fe350751d3",
    3: "b2d4d24bbe605d34b1098e0347db78b9cf7fe2d315bc94bc14b3e1342dbb0aaa",
    100: "baa7dbb145be1798a8063cf9d83c2d19517f36ba85a92cecaa5e9fb2d1288246",
}


def _digest(events):
    return hashlib.sha256(json.dumps(events, sort_keys=True).encode()).hexdigest()


@pytest.mark.parametrize("seed", sorted(DIGESTS))
def test_the_sharded_tests_scripts_are_the_recorded_ones(seed):
    events = regime_seq.script(seed, 5, extended=seed >= 100)
    assert _digest(events) == DIGESTS[seed], events
    assert all("metric" not in e for e in events)


@pytest.mark.parametrize("seed", sorted(DIGESTS))
def test_metrics_only_adds_a_key(seed):
    """metrics=True draws the objective from a generator of its own: every other key of every event is unchanged"""
    events = regime_seq.script(seed, 5, extended=seed >= 100, metrics=True)
    assert all(e["metric"] in (0, 1, 2) for e in events)
    assert _digest([{k: v for k, v in e.items() if k != "metric"} for e in events]) == DIGESTS[seed]


@pytest.mark.parametrize("seed", [4, 5, 125])
def test_the_symmetric_sharded_seeds_hold_the_mix_they_were_chosen_for(seed):
    events = regime_seq.script(seed, 5, extended=seed >= 100, metrics=True)
    m = [e["metric"] for e in regime_seq.solves(events)]
    assert m.count(2) >= 3, m
    assert any(a == 1 and b == 2 for a, b in zip(m, m[1:])) and any(a == 2 and b == 1 for a, b in zip(m, m[1:])), m
