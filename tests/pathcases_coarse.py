"""The size-selected paths of mvicp_coarse_pairs (csrc/coarse.hip), stated once for tests/test_coarse_paths_cpu.py and
tests/test_gpu_coarse_paths.py.  The constants are read from the sources by name (a name that is not found raises), and the host arithmetic
of coarse_pairs() -- the work table of the match launch and the work table of the scoring launch -- is restated here as small pure
functions of the sizes and those constants.  A case states the path it is built for as a condition on the plan, so a constant that changes
makes the case's own assertion fail instead of letting it drift off its path.

  match    per table (m left rows against n right rows): chunk = match_chunk, raised to ceil(n / kMaxChunks) when that many chunks would
           be exceeded, cut to n when larger; one record per (block of left rows, chunk); a chunk is walked in tiles of kTile / kGenTile rows
  score    slot_blocks = sum over edges of ceil(accepted_e / kThreads); want = ceil(kWantBlocks / slot_blocks) pair chunks per slot block,
           at most one per tile of kPairTile pairs; per_y = whole tiles; one record per (edge, slot block, pair chunk)
"""
import os
import re

import numpy as np

import pathcases as pc

COARSE_NAMES = ("kThreads", "kPairTile", "kWantBlocks", "kMaxChunks")
TILE_NAMES = ("kThreads", "kTile", "kGenRows", "kGenTile")
MATCH_RECORD_BYTES, SCORE_RECORD_BYTES = 40, 16


def load_constants(csrc=None):
    return {"coarse": pc.int_constants(pc.read_source("coarse.hip", csrc), COARSE_NAMES, "csrc/coarse.hip"),
            "tile": pc.int_constants(pc.read_source("match_tile.h", csrc), TILE_NAMES, "csrc/match_tile.h")}


CONSTANTS = load_constants()


def _cdiv(a, b):
    return -(-a // b)


def table_plan(match_chunk, m, n, dim, k=None):
    """one table of m left rows against n right rows -> dict(chunk, chunks, clamped, cut, tile, tiles_per_chunk, rows_in_last_tile_of_last_chunk,
    blocks, records)"""
    k = k or CONSTANTS
    left = k["tile"]["kThreads"] if dim == 33 else k["tile"]["kGenRows"]
    tile = k["tile"]["kTile"] if dim == 33 else k["tile"]["kGenTile"]
    if m == 0 or n == 0:
        return {"chunk": 1, "chunks": 0, "clamped": False, "cut": False, "tile": tile, "tiles_per_chunk": 0, "rows_in_last_tile_of_last_chunk": 0,
                "blocks": _cdiv(m, left), "records": 0}
    ch = match_chunk if match_chunk > 0 else 1
    clamped = _cdiv(n, ch) > k["coarse"]["kMaxChunks"]
    if clamped:
        ch = _cdiv(n, k["coarse"]["kMaxChunks"])
    cut = ch > n
    if cut:
        ch = n
    chunks = _cdiv(n, ch)
    last = n - (chunks - 1) * ch
    return {"chunk": ch, "chunks": chunks, "clamped": clamped, "cut": cut, "tile": tile, "tiles_per_chunk": _cdiv(ch, tile),
            "rows_in_last_tile_of_last_chunk": last - (_cdiv(last, tile) - 1) * tile, "blocks": _cdiv(m, left), "records": _cdiv(m, left) * chunks}


def tables_of(rows, edges, mutual):
    """the distinct ordered set pairs the edges need, in the order coarse_pairs() meets them"""
    out = []
    for a, b in edges:
        for t in ((a, b), (b, a)) if mutual else ((a, b),):
            if t not in out:
                out.append(t)
    return [(rows[a], rows[b]) for a, b in out]


def match_model_bytes(match_chunk, tables, dim, k=None):
    """the model bytes that coarse_pairs() books on the scope "coarse_match" """
    total, records = 0.0, 0
    for m, n in tables:
        p = table_plan(match_chunk, m, n, dim, k)
        total += 8.0 * dim * (float(m) * p["chunks"] + float(p["blocks"]) * n) + 24.0 * float(m) * p["chunks"]
        records += p["records"]
    return total + MATCH_RECORD_BYTES * float(records), records


def score_plan(pairs, accepted, k=None):
    """pairs / accepted per edge -> dict(slot_blocks, want, edges = [dict(gx, tiles, gy, per_y, records)], records)"""
    k = (k or CONSTANTS)["coarse"]
    slot_blocks = sum(_cdiv(a, k["kThreads"]) for a in accepted)
    if slot_blocks == 0:
        return {"slot_blocks": 0, "want": 0, "edges": [], "records": 0}
    want = _cdiv(k["kWantBlocks"], slot_blocks)
    edges = []
    for c, a in zip(pairs, accepted):
        if a <= 0:
            edges.append({"gx": 0, "tiles": 0, "gy": 0, "per_y": 0, "records": 0})
            continue
        tiles = _cdiv(c, k["kPairTile"])
        gy = min(want, tiles)
        per_y = _cdiv(tiles, gy) * k["kPairTile"]
        gx = _cdiv(a, k["kThreads"])
        edges.append({"gx": gx, "tiles": tiles, "gy": gy, "per_y": per_y, "tiles_per_record": per_y // k["kPairTile"], "records": gx * _cdiv(c, per_y)})
    return {"slot_blocks": slot_blocks, "want": want, "edges": edges, "records": sum(e["records"] for e in edges)}


def score_model_bytes(plan, pairs, accepted):
    """the model bytes that coarse_pairs() books on the scope "coarse_score" """
    return sum(48.0 * c * e["gx"] + 148.0 * a for c, a, e in zip(pairs, accepted, plan["edges"]) if a > 0) + SCORE_RECORD_BYTES * float(plan["records"])


# ---- the cases
# P1: more chunks than kMaxChunks would be: a long right operand at match_chunk = 1 (the backward table is cut to its two right rows)
P1_ROWS, P1_DIM, P1_CHUNK = (2, 65535 + 101), 7, 1
# P2: the chunk cut to the right operand: the default match_chunk over sets that are smaller, several tiles in the one chunk
P2_ROWS, P2_CHUNK = (257, 300), 2048
# P3: so many accepted hypotheses that a scoring record walks every tile of its edge (want = 1 < tiles)
P3_ROWS, P3_H, P3_EDGES = (300, 257), 180000, 3


def p1_sets():
    rng = np.random.Generator(np.random.PCG64(31))
    desc = rng.integers(0, 3, size=(sum(P1_ROWS), P1_DIM)).astype(np.float64)
    xyz = rng.uniform(0.0, 1.0, size=(sum(P1_ROWS), 3))
    return desc, xyz, np.array([0, P1_ROWS[0], sum(P1_ROWS)], dtype=np.int64)


def p3_sets():
    """two sets whose rows correspond one to one (distinct descriptors, a rigid motion and a little noise between the clouds)"""
    rng = np.random.Generator(np.random.PCG64(32))
    from mvicp import synth
    base_d = rng.uniform(0.0, 100.0, size=(300, 33))
    base_x = rng.uniform(0.0, 1.0, size=(300, 3))
    R, t = synth.so3_exp(rng.uniform(-1.0, 1.0, size=3)), rng.uniform(-0.5, 0.5, size=3)
    desc = np.concatenate([base_d[:P3_ROWS[0]], base_d[:P3_ROWS[1]]])
    xyz = np.concatenate([base_x[:P3_ROWS[0]], base_x[:P3_ROWS[1]] @ R.T + t + rng.normal(0.0, 0.01, size=(P3_ROWS[1], 3))])
    return np.ascontiguousarray(desc), np.ascontiguousarray(xyz), np.array([0, P3_ROWS[0], sum(P3_ROWS)], dtype=np.int64)
