"""No GPU: the constants that decide the paths of mvicp_coarse_pairs are found in the sources by name, and every case of
tests/pathcases_coarse.py lies on the path it is built for."""
import os
import shutil

import pytest

import pathcases as pc
import pathcases_coarse as pcc


def test_constants_are_read_from_the_sources_by_name(tmp_path):
    k = pcc.CONSTANTS
    assert set(k["coarse"]) == set(pcc.COARSE_NAMES) and set(k["tile"]) == set(pcc.TILE_NAMES)
    # the tile loops are shared: the launches of match.hip and of coarse.hip are written in the same tiling
    assert {n: k["tile"][n] for n in pcc.TILE_NAMES} == {n: pc.CONSTANTS["match"][n] for n in pcc.TILE_NAMES}
    assert k["coarse"]["kMaxChunks"] == pc.CONSTANTS["match"]["kMaxChunks"] and k["coarse"]["kPairTile"] == pc.CONSTANTS["consensus"]["kPairTile"]
    for name, old, new in (("coarse.hip", "kWantBlocks", "kBlocksWanted"), ("match_tile.h", "constexpr int kGenTile", "constexpr long kGenTile")):
        d = tmp_path / name.replace(".", "_")
        d.mkdir()
        for f in ("coarse.hip", "match_tile.h"):
            shutil.copy(os.path.join(pc.CSRC, f), d / f)
        text = (d / name).read_text()
        assert old in text
        (d / name).write_text(text.replace(old, new))
        with pytest.raises(LookupError):
            pcc.load_constants(str(d))


def test_the_match_cases_lie_on_their_paths():
    m, n = pcc.P1_ROWS
    fwd, bwd = pcc.table_plan(pcc.P1_CHUNK, m, n, pcc.P1_DIM), pcc.table_plan(pcc.P1_CHUNK, n, m, pcc.P1_DIM)
    assert fwd["clamped"] and not fwd["cut"] and fwd["chunk"] == 2 and fwd["chunks"] <= pcc.CONSTANTS["coarse"]["kMaxChunks"] and fwd["records"] == fwd["chunks"]
    assert not bwd["clamped"] and bwd["chunk"] == 1 and bwd["chunks"] == m and bwd["blocks"] > 1000
    assert pcc.tables_of(pcc.P1_ROWS, [(0, 1)], True) == [(m, n), (n, m)] and pcc.tables_of(pcc.P1_ROWS, [(0, 1), (1, 0), (0, 1)], True) == [(m, n), (n, m)]
    assert pcc.tables_of(pcc.P1_ROWS, [(0, 1), (0, 1)], False) == [(m, n)]
    for dim in (33, 7):
        a, b = pcc.P2_ROWS
        p = pcc.table_plan(pcc.P2_CHUNK, a, b, dim)
        assert p["cut"] and not p["clamped"] and p["chunks"] == 1 and p["tiles_per_chunk"] > 1 and 0 < p["rows_in_last_tile_of_last_chunk"] < p["tile"]
        assert p["blocks"] > 1
        e = pcc.table_plan(pcc.P2_CHUNK, a, 0, dim)
        assert e["records"] == 0 and e["blocks"] > 0   # (an empty right operand: no match record, the merge still pads the rows)


def test_the_scoring_plans():
    k = pcc.CONSTANTS["coarse"]
    few = pcc.score_plan([300, 257, 2, 0], [300, 1, 0, 0])   # few accepted: one record per tile
    assert few["want"] > 2 and [e["gy"] for e in few["edges"]] == [2, 2, 0, 0] and few["edges"][0]["tiles_per_record"] == 1 and few["records"] == 2 * 2 + 2
    acc = pcc.P3_H - 10   # (about what is accepted at edge_sim = 0)
    many = pcc.score_plan([300] * pcc.P3_EDGES, [acc] * pcc.P3_EDGES)
    assert many["slot_blocks"] >= k["kWantBlocks"] and many["want"] == 1
    assert all(e["gy"] == 1 and e["tiles_per_record"] == 2 and e["records"] == e["gx"] for e in many["edges"])
    two = pcc.score_plan([300] * 2, [acc] * 2)                # one edge fewer would split the pairs again
    assert two["want"] == 2
    assert pcc.score_plan([5, 5], [0, 0])["records"] == 0
