"""-m gpu: the launch order of the linearize workgroups (option lin_tail_last: every edge's full chunks first, all partial last chunks behind them)
changes no block.  A partial's slot is its chunk's place in its edge's run whatever the workgroup's place in the launch table, and the table's pads
return at once, so the bar between lin_tail_last 1 and 0 is byte for byte: all four flag combinations, the single and the paired launch, one symmetric
and one plane-to-plane evaluation.  The point and plane blocks are also held to the CPU oracle by the bar of
test_gpu_parity.py::test_linearize_explicit_correspondences_and_chunk_boundaries.

Graph: two edges of one source cloud (1->0, 1->2: interleaved in the table) and one edge of another (2->0); lin_chunk 512.  View sizes 2 x 512 + 3
(two full chunks and a tail per edge), 1024 (no tail) and 300 (a tail only); list lengths 1, 511, 512, 513, the full view (an identity list: the
shared-source-cloud path) and an empty edge, rotated over the three edges."""
import numpy as np
import pytest

import mvicp
from mvicp import synth
from mvicp.lib import METRIC_SYMMETRIC

pytestmark = pytest.mark.gpu

CHUNK = 512
SRC, DST = [1, 1, 2], [0, 2, 0]
FLAGS = [(1, 1), (1, 0), (0, 1), (0, 0)]   # (point_to_plane, robust)
A = 0.013


def _lists(N):
    """one triple of lists per case: the lengths 1, 511, 512, 513, N (those that fit) rotated over the edges, one edge of each case empty; then all full"""
    rng = np.random.default_rng(7)
    lens = [n for n in (1, CHUNK - 1, CHUNK, CHUNK + 1) if n < N] + [N]
    cases = []
    for i in range(len(lens)):
        case = []
        for e in range(3):
            n = 0 if e == i % 3 else lens[(i + e) % len(lens)]
            f = np.sort(rng.choice(N, n, replace=False)).astype(np.int32)
            s = rng.integers(0, N, n).astype(np.int32)
            case.append((f, s))
        cases.append(case)
    ident = np.arange(N, dtype=np.int32)      # and every edge full: both edges of source 1 read the shared sorted cloud side by side
    cases.append([(ident, rng.integers(0, N, N).astype(np.int32)) for _ in range(3)])
    return cases


def _evaluate(eng, Pa, Pb):
    out = {}
    for plane, robust in FLAGS:
        out["single", plane, robust] = eng.linearize(Pa, plane, robust)
        out["pair", plane, robust] = np.stack(eng.linearize_pair(Pa, Pb, plane, robust))
    out["sym"] = eng.linearize_metric(Pa, METRIC_SYMMETRIC, 1)
    out["gicp"] = eng.linearize_gicp(Pa, 1e-3, True)
    return out


@pytest.mark.parametrize("N", [2 * CHUNK + 3, 2 * CHUNK, 300])
def test_blocks_do_not_depend_on_the_launch_order(orc, N):
    pb = synth.make_problem(3, N)
    rng = np.random.default_rng(11)
    Pb = np.array([synth.add_noise(P, 2e-3, 1e-3, rng) for P in pb["init"]])
    cases = _lists(N)
    got = {}
    eng = mvicp.Engine(0)
    try:
        eng.set_option("lin_chunk", CHUNK)
        eng.set_frames(pb["pts"], pb["nor"])
        for tail_last in (1, 0):
            eng.set_option("lin_tail_last", tail_last)      # read at set_graph
            eng.set_graph(SRC, DST)
            for i, case in enumerate(cases):
                for e, (f, s) in enumerate(case):
                    eng.set_correspondences(e, f, s, A)
                got[tail_last, i] = _evaluate(eng, pb["init"], Pb)
    finally:
        eng.close()
    for i, case in enumerate(cases):
        new, old = got[1, i], got[0, i]
        lens = [len(f) for f, _ in case]
        for key in new:
            assert np.all(np.isfinite(new[key])), (N, lens, key)
            assert new[key].tobytes() == old[key].tobytes(), (N, lens, key, float(np.abs(new[key] - old[key]).max()))
        for e, n in enumerate(lens):
            if n == 0:
                for key in new:
                    assert not np.any(new[key][..., e, :]), (N, lens, key, e)
        for plane, robust in FLAGS:
            assert new["pair", plane, robust][0].tobytes() == new["single", plane, robust].tobytes(), (N, lens, plane, robust)
            for poses, blocks in ((pb["init"], new["single", plane, robust]), (Pb, new["pair", plane, robust][1])):
                want = orc.edge_blocks(pb["pts"], pb["nor"], SRC, DST, case, [np.float32(A)] * 3, poses, plane, robust)
                for e, n in enumerate(lens):
                    if n == 0:
                        continue
                    scale = np.abs(want[e, :78]).max()
                    assert np.allclose(blocks[e], want[e], rtol=1e-10, atol=1e-11 * scale), (N, lens, plane, robust, e)
