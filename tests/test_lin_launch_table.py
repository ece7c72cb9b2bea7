"""CPU: the launch table of the linearization's workgroups (mv-lm-icp_amd/csrc/lin_table.h through tests/lin_table_harness.cpp, compiled with g++;
options lin_interleave, lin_tail_last).  The table only orders the chunks of a launch, so what has to hold is structural: every chunk of every edge
exactly once; every other entry a pad that starts at or past its edge's end (its workgroup returns before it touches memory); with lin_tail_last 0
the order the library had before the option existed; with lin_tail_last 1 that SAME table up to its length with every partial chunk replaced by a
pad (every full chunk keeps its entry, and so its XCD), then all partial chunks, those of two edges of one source cloud a multiple of 8 entries
apart (the same XCD), and no pad at the very end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRAPHS = {
    # name: (src per edge, n_src per edge, chunk)
    "cfg4": ([1 + i // 2 for i in range(62)], [200_000] * 62, 8192),
    "three_edges": ([1, 1, 2], [1027, 1027, 1027], 512),
    "no_tail": ([1, 1, 2], [1024, 1024, 512], 512),
    "tail_only": ([1, 1, 2, 3], [300, 300, 1, 511], 512),
    "mixed": ([0, 0, 0, 1, 2, 2, 3, 4, 4, 5, 6, 7, 8, 8, 9, 9, 9], [5000, 5000, 5000, 4096, 100, 100, 0, 777, 777, 4097, 12, 513, 9000, 9000, 1, 1, 1], 512),
    "unowned": ([1, 1, 2, 2, 3, 3], [0, 0, 3000, 0, 3000, 3000], 1024),     # edges of other ranks hold no source points here
    "one_edge": ([1], [9001], 4096),
    "empty": ([], [], 512),
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lin_table") / "lin_table_harness.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "lin_table_harness.cpp")], timeout=300)
    lib = C.CDLL(so)
    ip = C.POINTER(C.c_int)
    lib.lin_table.argtypes = [C.c_int, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]

    def call(src, n_src, chunk, interleave, tail_last):
        src, n_src = np.ascontiguousarray(src, dtype=np.int32), np.ascontiguousarray(n_src, dtype=np.int32)
        cap = int(sum(-(-int(n) // chunk) + 9 for n in n_src)) + 8     # every chunk, a pad in the place of a partial one, the pads of the tail section
        ce, cs = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
        n = lib.lin_table(len(src), src.ctypes.data_as(ip), n_src.ctypes.data_as(ip), chunk, interleave, tail_last, cap, ce.ctypes.data_as(ip), cs.ctypes.data_as(ip))
        assert 0 <= n <= cap, (n, cap)
        return list(zip(ce[:n].tolist(), cs[:n].tolist()))
    return call


def _before_the_option(src, n, chunk, interleave):
    """the order without lin_tail_last: edge by edge, or the chunks of one source cloud's edges interleaved in groups of 8"""
    nch = [-(-x // chunk) for x in n]
    out = []
    e0 = 0
    while e0 < len(src):
        e1 = e0 + 1
        while interleave and e1 < len(src) and src[e1] == src[e0]:
            e1 += 1
        for g in range(0, max(nch[e0:e1]), 8):
            for e in range(e0, e1):
                out += [(e, k * chunk) for k in range(g, min(g + 8, nch[e]))]
        e0 = e1
    return out


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("interleave", [1, 0])
@pytest.mark.parametrize("tail_last", [1, 0])
def test_table_holds_every_chunk_once_and_pads_past_the_end(table, name, interleave, tail_last):
    src, n, chunk = GRAPHS[name]
    entries = table(src, n, chunk, interleave, tail_last)
    assert all(0 <= e < len(src) and s >= 0 and s % chunk == 0 for e, s in entries)
    real = [(e, s) for e, s in entries if s < n[e]]
    want = [(e, k * chunk) for e in range(len(src)) for k in range(-(-n[e] // chunk))]
    assert sorted(real) == want                                  # every chunk, once
    old = _before_the_option(src, n, chunk, interleave)
    if not tail_last:
        assert entries == old
        return
    if entries:
        assert entries[-1][1] < n[entries[-1][0]]                # no pad at the end
    partial = lambda e, s: s < n[e] < s + chunk                  # noqa: E731
    n_part = sum(1 for e, s in old if partial(e, s))
    head, tail = entries[:len(old)], entries[len(old):]
    if n_part == 0:
        assert entries == old                                    # nothing to move
        return
    assert len(head) == len(old)
    for (e, s), (eo, so) in zip(head, old):                      # every full chunk where it was; a pad on the partial chunk's own edge in its place
        assert e == eo and (s >= n[e] if partial(eo, so) else s == so), ((e, s), (eo, so))
    assert sum(1 for e, s in tail if s < n[e]) == n_part
    assert all(partial(e, s) or s >= n[e] for e, s in tail)      # the workgroups that start last are the short ones
    if not interleave:
        assert [x for x in tail] == [(e, n[e] // chunk * chunk) for e in range(len(src)) if n[e] % chunk]
        return
    assert len(tail) <= 8 * len(src)
    where = {x: i for i, x in enumerate(tail)}
    for e in range(1, len(src)):
        if src[e] == src[e - 1] and n[e] % chunk and n[e - 1] % chunk:
            a, b = where[(e - 1, n[e - 1] // chunk * chunk)], where[(e, n[e] // chunk * chunk)]
            assert b > a and (b - a) % 8 == 0, (e, a, b)


def test_cfg4_table(table):
    src, n, chunk = GRAPHS["cfg4"]
    t = table(src, n, chunk, 1, 1)
    assert len(t) == 62 * 25 + 62 + 1                           # the table without the option (62 pads in it), 62 last chunks, and one pad: 31 source clouds = 3 batches of 8 and one of 7
    assert [e for e, _ in t[:16]] == [0] * 8 + [1] * 8 and [s for _, s in t[:8]] == [k * chunk for k in range(8)]      # A0..A7, B0..B7
    assert t[48:50] == [(0, 25 * chunk), (1, 25 * chunk)] and t[50] == (2, 0)                                         # pads where A24, B24 were: the next source starts at entry 50
    assert [e for e, _ in t[1550:1566]] == list(range(0, 16, 2)) + list(range(1, 16, 2)) and all(s == 24 * chunk for _, s in t[1550:1566])
    assert sum(1 for e, s in t[1550:] if s >= n[e]) == 1
