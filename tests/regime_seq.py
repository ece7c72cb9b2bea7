"""A scripted registration whose rounds cross every regime of mvicp_correspond (TEST INFRASTRUCTURE): cutoff changes, fixed-mask changes,
mvicp_reset_history, forced kernel methods, option flips and rounds without a solve (bit-identical poses), drawn from a seeded generator —
every rank of a sharded job and the single process it is compared with replay the SAME script.  After every round the runner records
(counts, weight bits, poses): with N > 1 ranks the skip / arm decisions of mvicp_correspond (tie_skip, far_skip, spec_arm, the bracket
select, list reuse) are taken per rank from exchanged data, and every rank's record must equal the single process's bit for bit
(tests/test_gpu_multirank.py: host-staged transport on one GPU; tests/test_gpu_rccl2.py: RCCL on two GPUs)."""
import numpy as np


KINDS = ["none", "none", "cutoff", "fixed", "reset", "method", "option", "hold", "hold"]
# extended scripts: a search that FAILS before the round's search (an unknown nn_method, or an injected launch failure that every rank
# meets: all of them enter the exchange poisoned), at poses of its own, and flips of the tie rule
KINDS_EXTENDED = KINDS + ["fail", "fail", "tie_rule", "tie_rule"]


def script(seed, K, rounds=14, extended=False, metrics=False):
    """-> list of per-round event dicts (pure function of its arguments).  extended=False draws exactly the sequences it always drew.
    metrics=True adds e["metric"] in {0 POINT, 1 PLANE, 2 SYMMETRIC} to every event, drawn from a generator of its own: every other key is
    what the same call without it gives (tests/test_regime_script_cpu.py holds the scripts of the sharded tests to a recorded digest)."""
    rng = np.random.default_rng(4200 + seed)
    rng_metric = np.random.default_rng(77000 + seed)
    ev = []
    for rnd in range(rounds):
        kind = str(rng.choice(KINDS_EXTENDED if extended else KINDS)) if rnd > 0 else "none"
        e = {"kind": kind}
        if kind == "cutoff":
            e["cutoff"] = float(rng.choice([0.05, 0.02, 0.008]))
        elif kind == "fixed":
            e["frame"] = int(rng.integers(1, K))
        elif kind == "method":
            e["method"] = int(rng.choice([0, 0, 1, 2, 3]))          # AUTO, AUTO, BRUTE, GRID, TILE
        elif kind == "option":
            e["name"] = str(rng.choice(["list_reuse", "nn_cache", "sel_bracket", "tile_cache", "tile_seed", "tile_miss", "mfma_entry", "reject_cache"]))
            e["value"] = float(rng.integers(0, 2)) * (8.0 if e["name"] == "tile_miss" else 1.0)
        elif kind == "fail":
            e["inject"] = bool(rng.integers(0, 2)); e["frame"] = int(rng.integers(1, K)); e["shift"] = [float(v) for v in rng.normal(0.0, 2e-3, 3)]
            e["retry_there"] = bool(rng.integers(0, 2))
        e["param"] = int(rng.integers(0, 3)); e["plane"] = int(rng.integers(0, 2)); e["robust"] = bool(rng.integers(0, 2))
        if metrics:
            e["metric"] = int(rng_metric.integers(0, 3))
        ev.append(e)
    return ev


def solves(events):
    """the events whose round ends with a solve (run() below: every kind but "hold" and "fail"), in order"""
    return [e for e in events if e["kind"] not in ("hold", "fail")]


def run(eng, pb, events, after_search=None, after_round=None, masks=None):
    """Replays `events` on an engine that already holds the clouds and the graph.  -> list of (counts, weights-as-bytes, poses) per round.
    Hooks (tests/test_gpu_sym_regimes.py; the sharded tests use none): after_search(state) runs between the round's search and its solve,
    after_round(state) after the solve; state = {"round", "event", "poses", "fixed", "cutoff", "method", "options", "counts", "weights"}, the
    round's own values ("options": what the script has set so far).  A kind the scripts above never draw, for hand-written events: "normals"
    (mvicp_recompute_normals(frame, 10) before the round's search; the new normals go to state["normals"]).  And a metric they never draw: 3, the
    plane-to-plane objective — the round's solve is mvicp_optimize_gicp at e["epsilon"] (default 1e-3; tests/test_gpu_gicp_regimes.py).
    Another hand-written kind: "mask" (tests/maskcases.py) — eng.set_reject_mask(e["frame"], e["mask"], e["roles"]) before the round's search; the
    round is otherwise a "none" round.  state["masks"]: per frame the (mask, roles) currently set, (None, 0) for none; `masks` = {frame: (mask,
    roles)}: what the caller has set on the engine before the call."""
    poses = pb["init"].copy()
    fixed = pb["fixed"].copy()
    cutoff, method, rule = 0.05, 0, 1
    options = {}
    cur_masks = {f: (None, 0) for f in range(len(pb["pts"]))}
    cur_masks.update(masks or {})
    out = []
    for rnd, e in enumerate(events):
        k = e["kind"]
        state = {"round": rnd, "event": e}
        if k == "cutoff":
            cutoff = e["cutoff"]
        elif k == "fixed":
            fixed[e["frame"]] = 1 - fixed[e["frame"]]
        elif k == "reset":
            eng.reset_history()
        elif k == "method":
            method = e["method"]
        elif k == "option":
            eng.set_option(e["name"], e["value"])
            options[e["name"]] = e["value"]
        elif k == "normals":
            state["normals"] = eng.recompute_normals(e["frame"], 10)
        elif k == "mask":
            eng.set_reject_mask(e["frame"], e["mask"], e["roles"])
            cur_masks[e["frame"]] = (e["mask"], e["roles"]) if (e["mask"] is not None and e["roles"]) else (None, 0)
        elif k == "tie_rule":
            rule = 1 - rule
            eng.set_option("tie_rule", rule)
        elif k == "fail":
            Pf = poses.copy()
            Pf[e["frame"]][:3, 3] += np.array(e["shift"])
            if e["inject"]:
                eng.set_option("fault_inject", 1)
            try:
                eng.correspond(Pf, fixed, cutoff, method if e["inject"] else 99)
            except RuntimeError:                              # (mvicp.MvicpError)
                pass
            else:
                raise AssertionError("the scripted failing search did not fail")
            if e["retry_there"]:
                poses = Pf
        counts, weights = eng.correspond(poses, fixed, cutoff, method)
        state.update(poses=poses, fixed=fixed.copy(), cutoff=cutoff, method=method, options=dict(options), counts=counts.copy(), weights=weights.copy(),
                     masks=dict(cur_masks))
        if after_search is not None:
            after_search(state)
        if k not in ("hold", "fail") and counts.sum() > 0:
            if e.get("metric") == 3:       # hand-written events only (script() draws 0, 1, 2): the plane-to-plane objective, which has no mvicp_metric value
                poses, _ = eng.optimize_gicp(poses, fixed, e["param"], e.get("epsilon", 1e-3), e["robust"], 50)
            elif "metric" in e:
                poses, _ = eng.optimize_metric(poses, fixed, e["param"], e["metric"], e["robust"], 50)
            else:
                poses, _ = eng.optimize(poses, fixed, e["param"], e["plane"], e["robust"], 50)
        out.append((counts.copy(), weights.tobytes(), poses.copy()))
        if after_round is not None:
            state["poses"] = poses
            after_round(state)
    return out


def save(path, log):
    np.savez(path, counts=np.array([l[0] for l in log]), weights=np.array([np.frombuffer(l[1], dtype=np.float32) for l in log]), poses=np.array([l[2] for l in log]))


def assert_equal(path, log, tag):
    z = np.load(path)
    for r, (c, w, P) in enumerate(log):
        assert np.array_equal(z["counts"][r], c), (tag, r, "counts")
        assert z["weights"][r].tobytes() == w, (tag, r, "weights")
        assert np.array_equal(z["poses"][r], P), (tag, r, float(np.abs(z["poses"][r] - P).max()))
