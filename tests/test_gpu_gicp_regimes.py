"""-m gpu: the plane-to-plane blocks against the extended-precision reference THROUGH a scripted registration.

The sibling of tests/test_gpu_sym_regimes.py.  linearize_gicp_kernel runs in the pipeline it shares with the symmetric kernel (csrc/lin_normal.h)
but takes the other branch of its one switch (LO_SCALAR: the 12 low parts of the relative transform by scalar loads before the barrier, from a
block-uniform address) and has an accumulate step of its own; tests/test_gpu_gicp_accuracy.py meets a `first` that is not the identity only
through explicit lists on a fresh context.  Here one engine replays the sixteen hand-written rounds of the symmetric test (its tail(): inactive
edges with stale full lists, explicit permuted lists, compaction gaps, list reuse on and off, lin_share_p 0 and 1, mvicp_recompute_normals on a
source and on a destination), after the two rounds that lead to the tail's starting state: a first searched round, then frame 2 fixed.  EVERY
solve is mvicp_optimize_gicp at epsilon = 1e-3 (regime_seq.run, metric 3).  AFTER EVERY ROUND every edge's list is fetched and
mvicp_linearize_gicp(1e-3), robust on and off, is held to gicpref.edge_block on that list — with the normals in force, recomputed ones included —
by the bar of the accuracy sweep (its MARGIN, _judge and _references).  An edge whose list is empty must give an all-zero block.  All nine STATES
of the symmetric test must be reached.  These are real surface normals at nearly converged poses: the near-parallel regime on real data.  The
worst ratio of every round is printed."""
import hashlib

import numpy as np
import pytest

import gicpref
import mvicp
import regime_seq
from mvicp import synth
from test_gpu_gicp_accuracy import MARGIN, _judge, _references
from test_gpu_sym_regimes import EXPLICIT_EDGE, K, N, STATES, _ev, reached_states, tail

pytestmark = pytest.mark.gpu

EPS = 1e-3
GICP = 3          # regime_seq.run's value for mvicp_optimize_gicp


def events():
    lead = [_ev("none", GICP), _ev("fixed", GICP, frame=2)]          # a first searched round, then frame 2 fixed: where the tail starts
    return lead + [dict(e, metric=GICP) for e in tail()]


@pytest.mark.parametrize("interleave", [1, 0], ids=["lin_interleave=1", "lin_interleave=0"])
def test_gicp_blocks_belong_to_the_lists_after_every_round_of_a_scripted_registration(interleave):
    pb = synth.make_problem(K, N)
    src, dst = [int(s) for s in pb["src"]], [int(d) for d in pb["dst"]]
    E = len(src)
    assert (src[EXPLICIT_EDGE], dst[EXPLICIT_EDGE]) == (3, 2)
    pts = pb["pts"]
    nor = [np.array(n) for n in pb["nor"]]
    a = np.zeros(E, dtype=np.float32)           # the scale of every edge's current list
    rec, failures = [], []
    rng = np.random.default_rng(1234)
    eng = mvicp.Engine(0)

    def after_search(st):
        e = st["event"]
        if "normals" in st:
            nor[e["frame"]] = st["normals"]
        a[:] = st["weights"]
        st["explicit"] = None
        if e.get("explicit"):
            f, s, _ = eng.get_correspondences(EXPLICIT_EDGE)
            assert len(f) == N and np.array_equal(f, np.arange(N))           # (this round's cutoff passes every query)
            perm = rng.permutation(N).astype(np.int32)
            eng.set_correspondences(EXPLICIT_EDGE, perm, s[perm], float(a[EXPLICIT_EDGE]))
            assert not np.array_equal(perm, np.arange(N))
            st["explicit"], st["explicit_second"] = perm, s

    def after_round(st):
        worst = 0.0
        lens = []
        blocks = {r: eng.linearize_gicp(st["poses"], EPS, r) for r in (1, 0)}
        for e in range(E):
            f, s, _ = eng.get_correspondences(e)
            lens.append(len(f))
            if st["fixed"][src[e]]:
                assert len(f) == 0, (st["round"], e)
            if e == EXPLICIT_EDGE and st["explicit"] is not None:
                assert np.array_equal(f, np.arange(N)) and np.array_equal(s, st["explicit_second"])      # (an explicit list comes back sorted by `first`)
            if len(f) == 0:
                for r in (1, 0):
                    assert not np.any(blocks[r][e]), (st["round"], e, r, blocks[r][e])
                continue
            operands = (pts[src[e]][f], pts[dst[e]][s], nor[dst[e]][s], nor[src[e]][f], st["poses"][src[e]], st["poses"][dst[e]])
            key = hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in operands + (np.float64(a[e]),))).digest()
            refs = _references(*operands, a[e], EPS, key)
            for r in (1, 0):
                before = len(failures)
                _judge(blocks[r][e], refs[r][0], refs[r][1], "round %d edge %d (%d)" % (st["round"], e, len(f)), EPS, r, failures)
                ratio = failures[-1][4] if len(failures) > before else gicpref.worst_ratio(gicpref.piece_errors(gicpref.unpack(blocks[r][e]), refs[r][0]), refs[r][1])[0]
                worst = max(worst, ratio)
        ev = st["event"]
        print("GICPREG interleave=%d round %2d %-8s fixed %s cutoff %-5g lists %s  worst ratio %.2f" % (
            interleave, st["round"], ev["kind"], st["fixed"].tolist(), st["cutoff"], lens, worst))
        rec.append(dict(kind=ev["kind"], event=ev, fixed=st["fixed"], cutoff=st["cutoff"], method=st["method"], lens=lens, worst=worst, explicit=st["explicit"] is not None,
                        reuse=st["options"].get("list_reuse", 1.0), share=st["options"].get("lin_share_p", 1.0)))

    try:
        eng.set_option("lin_interleave", interleave)      # read at set_graph
        eng.set_frames(pts, nor); eng.set_graph(src, dst)
        regime_seq.run(eng, pb, events(), after_search=after_search, after_round=after_round)
    finally:
        eng.close()

    reached = reached_states(rec, src, dst)
    assert reached == set(STATES), sorted(set(STATES) - reached)
    assert all(e["metric"] == GICP for e in events()) and len(regime_seq.solves(events())) >= 15
    assert len(rec) == len(events()) == 18
    assert MARGIN == 32.0
    assert not failures, failures
