"""The builds of the two tile NN kernels that the host picks from the DEPTH of the target's 64-wide box hierarchy, and cases that reach
each of them.  Test infrastructure only, in the manner of tests/pathcases.py.

The tile constants and the arms of the two dispatch lambdas (csrc/nn_tile.hip:launch_nn_tile_edges, csrc/nn_mfma.hip:launch_nn_mfma_edges)
are read from the project's sources by name (a name that is not found raises), `levels(n)` restates csrc/nn_tile.hip:build_wide, and
VARIANTS says for every launch string (mvicp_last_nn_launch) which options, method and kind of round reach it.
tests/test_depth_dispatch_cpu.py holds the table against the source without a GPU: an arm that needs a 3-level target (or the generic
build of a mixed-depth launch) and has no entry fails there, and so does an entry without an arm.  tests/test_gpu_nn_depth3.py runs the
table.  Every case generator is seeded with PCG64 and states its properties (size, exact ties, duplicates), which the CPU test holds."""
import os
import re

import numpy as np

import offorigin as oo
from mvicp import lib as L
from mvicp import synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mv-lm-icp_amd", "csrc")


# ---- the constants and the arms, from the sources
def read_source(name, csrc=None):
    with open(os.path.join(csrc or CSRC, name)) as f:
        return f.read()


def tile_constants(text, where="csrc/nn_tile_common.h"):
    """{"LEAF", "FAN"}: `#define MVICP_TILE_LEAF N` (the default of the tuning override) and `constexpr int FAN = N;`"""
    leaf = re.findall(r"^#define\s+MVICP_TILE_LEAF\s+(\d+)\s*$", text, flags=re.M)
    fan = re.findall(r"constexpr\s+int\s+FAN\s*=\s*(\d+)\s*;", text)
    if len(leaf) != 1 or len(fan) != 1:
        raise LookupError("%s: MVICP_TILE_LEAF found %d times, FAN %d times" % (where, len(leaf), len(fan)))
    return {"LEAF": int(leaf[0]), "FAN": int(fan[0])}


def levels(n, k=None):
    """box levels of a target of n points, as build_wide counts them: tiles of LEAF points, then FAN boxes per node until one node holds all"""
    k = k or CONSTANTS
    cnt = -(-n // k["LEAF"])
    lv = 1
    while cnt > k["FAN"]:
        cnt = -(-cnt // k["FAN"])
        lv += 1
    return lv


def _dispatch_body(text, fn, where):
    """the text of `int fn(...) { ... }` (a function at namespace scope: it ends at the first line that is a lone closing brace)"""
    start = text.find("\nint %s(" % fn)
    if start < 0:
        raise LookupError("%s: `int %s(` not found" % (where, fn))
    end = text.find("\n}\n", start)
    if end < 0:
        raise LookupError("%s: the end of %s not found" % (where, fn))
    return text[start:end]


_BOOL = {"true": 1, "false": 0}


def _arms(body, macro, nargs, where):
    """the argument tuples of every use of `macro(...)` in the dispatch (its #define and #undef lines excluded); every use must parse"""
    lines, in_macro = [], False
    for ln in body.split("\n"):
        if in_macro or re.match(r"\s*#\s*(define|undef)\b", ln):
            in_macro = ln.rstrip().endswith("\\")      # a definition goes on while its lines end in a backslash
            continue
        lines.append(re.sub(r"//.*", "", ln))
    code = "\n".join(lines)
    uses = len(re.findall(r"\b%s\s*\(" % macro, code))
    pat = r"\b%s\s*\(\s*(\d+)\s*,\s*(-?\d+)" % macro + r"\s*,\s*(true|false)" * (nargs - 2) + r"\s*\)"
    found = re.findall(pat, code)
    if len(found) != uses:
        raise LookupError("%s: %d uses of %s, %d with literal arguments" % (where, uses, macro, len(found)))
    return [(int(f[0]), int(f[1])) + tuple(_BOOL[b] for b in f[2:]) for f in found], code


def tile_arms(text, where="csrc/nn_tile.hip"):
    """the launch strings of launch_nn_tile_edges' arms, in source order: "tile<WPE,TOP,BND>" """
    body = _dispatch_body(text, "launch_nn_tile_edges", where)
    arms, code = _arms(body, "MVICP_TILE_K", 3, where)
    if not arms or "hipLaunchKernelGGL" in code:
        raise LookupError("%s: the dispatch of launch_nn_tile_edges has %d MVICP_TILE_K arms%s" % (where, len(arms), " and a launch that names no arm" if arms else ""))
    return ["tile<%d,%d,%d>" % a for a in arms]


def mfma_arms(text, where="csrc/nn_mfma.hip"):
    """the launch strings of launch_nn_mfma_edges' arms: "mfma<WPE,TOP,BND,CEN,LBT,ENTRY>".  MVICP_MFMA_L(W, T, B, C, Lb) is one build,
    MVICP_MFMA_E(W, T, B, C) the ENTRY build, MVICP_MFMA_K(W, T, B) the pair with and without the census."""
    body = _dispatch_body(text, "launch_nn_mfma_edges", where)
    out = []
    la, code = _arms(body, "MVICP_MFMA_L", 5, where)
    ea, _ = _arms(body, "MVICP_MFMA_E", 4, where)
    ka, _ = _arms(body, "MVICP_MFMA_K", 3, where)
    if not (la and ea and ka) or "hipLaunchKernelGGL" in code or "MVICP_MFMA_X" in code:
        raise LookupError("%s: the dispatch of launch_nn_mfma_edges has %d / %d / %d arms of MVICP_MFMA_L / _E / _K, or a launch that names no arm" % (where, len(la), len(ea), len(ka)))
    out += ["mfma<%d,%d,%d,%d,%d,0>" % a for a in la]
    out += ["mfma<%d,%d,%d,%d,0,1>" % a for a in ea]
    for w, t, b in ka:
        out += ["mfma<%d,%d,%d,%d,0,0>" % (w, t, b, c) for c in (0, 1)]
    if len(set(out)) != len(out):
        raise LookupError("%s: an instantiation is launched by two arms: %r" % (where, sorted(x for x in set(out) if out.count(x) > 1)))
    return out


def parse_launch(s):
    """{"kernel", "WPE", "TOP", "BND", "CEN", "LBT", "ENTRY"} of a launch string ("grid" / "brute": the kernel alone)"""
    m = re.fullmatch(r"(tile|mfma)<(-?\d+(?:,-?\d+)*)>", s)
    if not m:
        if s in ("grid", "brute"):
            return {"kernel": s}
        raise ValueError("not a launch string: %r" % (s,))
    v = [int(x) for x in m.group(2).split(",")]
    names = ("WPE", "TOP", "BND") if m.group(1) == "tile" else ("WPE", "TOP", "BND", "CEN", "LBT", "ENTRY")
    if len(v) != len(names):
        raise ValueError("not a launch string: %r" % (s,))
    return dict(zip(names, v), kernel=m.group(1))


def load_arms(csrc=None):
    return tile_arms(read_source("nn_tile.hip", csrc)) + mfma_arms(read_source("nn_mfma.hip", csrc))


def required_arms(arms):
    """the arms this table must cover: every build for 3-level targets (TOP = 2) and every generic build (TOP = -1: mixed depths)"""
    return [a for a in arms if parse_launch(a)["TOP"] in (2, -1)]


CONSTANTS = tile_constants(read_source("nn_tile_common.h"))
ARMS = load_arms()

# the smallest target with 3 box levels, and the sizes of the ragged end (tests/test_gpu_nn_depth3.py b)
N3 = CONSTANTS["LEAF"] * CONSTANTS["FAN"] ** 2 + 1
RAGGED_SIZES = (N3, N3 + CONSTANTS["LEAF"], N3 + CONSTANTS["LEAF"] * CONSTANTS["FAN"])

# ---- launch string -> how it is reached
# options on top of OPTION_DEFAULTS, the method, the kind of round, whether the census counts, and the depth of the targets:
#   "first"  : the first search after mvicp_reset_history (no seed anywhere)
#   "repeat" : the search after it, at the same poses (seeded; never cache-aware: every transform is bit-identical)
#   "cached" : a search after a bounds-leaving one at moved poses, with "tile_cache" 2 (the temporal-cache prologue runs)
#   depth 3 = every target has 3 levels, "mixed" = targets of 3, 2 and 1 levels in one launch, 2 = every target has 2 levels
OPTION_DEFAULTS = {"tile_mfma": 1, "tile_waves": 0, "tile_bounds": 1, "tile_cache": 1, "tile_miss": 8, "reject_cache": 1, "mfma_lbt": 1, "mfma_entry": 0, "nn_census": 0}


def _v(opts, kind, census=0, depth=3, method=L.NN_TILE):
    return {"opts": opts, "method": method, "round": kind, "census": census, "depth": depth}


_T0, _T2 = {"tile_mfma": 0}, {"tile_mfma": 2}
VARIANTS = {
    # nn_tile_kernel, 3 levels
    "tile<7,2,0>": _v(_T0, "first"),
    "tile<8,2,0>": _v(dict(_T0, tile_waves=8), "first"),
    "tile<6,2,0>": _v(dict(_T0, tile_waves=6), "repeat"),
    "tile<6,2,1>": _v(dict(_T0, tile_bounds=2), "first"),
    # nn_mfma_kernel, 3 levels: the unseeded per-lane-box builds, the seeded default, the occupancy variants (an unseeded launch never
    # reaches them while "mfma_lbt" is on), the bounds-leaving builds, the seed-block entry, the cache-aware per-lane-box build
    "mfma<5,2,0,0,1,0>": _v(_T2, "first"),
    "mfma<5,2,0,1,1,0>": _v(_T2, "first", census=1),
    "mfma<5,2,0,0,0,0>": _v(dict(_T2, mfma_lbt=0), "first"),
    "mfma<5,2,0,1,0,0>": _v(_T2, "repeat", census=1),
    "mfma<6,2,0,0,0,0>": _v(dict(_T2, tile_waves=6), "repeat"),
    "mfma<6,2,0,1,0,0>": _v(dict(_T2, tile_waves=6, mfma_lbt=0), "first", census=1),
    "mfma<4,2,0,0,0,0>": _v(dict(_T2, tile_waves=4, mfma_lbt=0), "first"),
    "mfma<4,2,0,1,0,0>": _v(dict(_T2, tile_waves=4), "repeat", census=1),
    "mfma<5,2,1,0,0,0>": _v(dict(_T2, tile_bounds=2), "first"),
    "mfma<5,2,1,1,0,0>": _v(dict(_T2, tile_bounds=2), "repeat", census=1),
    "mfma<5,2,0,0,0,1>": _v(dict(_T2, mfma_entry=1), "repeat"),
    "mfma<5,2,0,1,0,1>": _v(dict(_T2, mfma_entry=1), "repeat", census=1),
    "mfma<5,2,1,0,0,1>": _v(dict(_T2, mfma_entry=1, tile_bounds=2), "repeat"),
    "mfma<5,2,1,0,1,0>": _v(dict(_T2, tile_bounds=2, tile_cache=2, mfma_lbt=2), "cached"),
    # the generic builds: targets of 3, 2 and 1 levels in one launch
    "tile<6,-1,0>": _v(_T0, "first", depth="mixed"),
    "tile<8,-1,0>": _v(dict(_T0, tile_waves=8), "repeat", depth="mixed"),
    "tile<6,-1,1>": _v(dict(_T0, tile_bounds=2), "first", depth="mixed"),
    "mfma<5,-1,0,0,0,0>": _v(_T2, "first", depth="mixed"),
    "mfma<5,-1,0,1,0,0>": _v(_T2, "repeat", census=1, depth="mixed"),
    "mfma<5,-1,1,0,0,0>": _v(dict(_T2, tile_bounds=2), "repeat", depth="mixed"),
    "mfma<5,-1,1,1,0,0>": _v(dict(_T2, tile_bounds=2), "first", census=1, depth="mixed"),
    # the 2-level builds (tests/test_gpu_nn_offorigin.py runs them through the same one-edge route)
    "tile<6,1,0>": _v(_T0, "first", depth=2),
    "mfma<5,1,0,0,0,0>": _v(_T2, "first", depth=2),
    "mfma<5,1,0,1,0,0>": _v(_T2, "repeat", census=1, depth=2),
}


def variants(depth, rounds=("first", "repeat")):
    """[(launch string, variant)] of one depth, in the table's order"""
    return [(k, v) for k, v in VARIANTS.items() if v["depth"] == depth and v["round"] in rounds]


def apply_variant(eng, v):
    """the variant's options on top of the defaults (every option the table touches is set, so the order of variants does not matter)"""
    for k, d in OPTION_DEFAULTS.items():
        if k != "nn_census":
            eng.set_option(k, v["opts"].get(k, d))
    eng.profile(bool(v["census"]))
    eng.set_option("nn_census", v["census"])


def search_variant(eng, v, poses, fixed, thresh):
    """run a "first" or a "repeat" variant: yields (round, counts, weights, launch string) after each of its one or two searches, so that
    the caller reads the lists of each"""
    assert v["round"] in ("first", "repeat")
    eng.reset_history()
    apply_variant(eng, v)
    for r in range(2 if v["round"] == "repeat" else 1):
        c, w = eng.correspond(poses, fixed, thresh, v["method"])
        yield r, c, w, eng.last_nn_launch()


# ---- the one-edge route: an arbitrary query set through a tile kernel
def edge_frames(targets, q):
    """frames [targets..., queries], one edge from the queries to every target, identity poses (the query map is exact), the queries free"""
    t = list(targets)
    src = np.full(len(t), len(t), dtype=np.int32)
    dst = np.arange(len(t), dtype=np.int32)
    fixed = np.array([1] * len(t) + [0], dtype=np.uint8)
    return t + [np.ascontiguousarray(q, dtype=np.float64)], src, dst, np.stack([np.eye(4)] * (len(t) + 1)), fixed


def cutoff_above(d2):
    """a float32 cutoff above every distance of the query set (twice the largest)"""
    return np.float32(2.0 * np.sqrt(float(np.max(d2))) + 1e-30)


def expected_list(orc, idx, d2, thresh):
    """the reference's list (first, second, dist, weight) from the oracle's answers; the cutoff must keep every query"""
    f, s, d, w = orc.filter_median(idx, d2, thresh)
    assert len(f) == len(idx), "the cutoff must lie above every distance"
    return f, s, d, w


# ---- the clouds
KINDS = ("blob", "plane", "lattice", "clusters")
OTHER_KIND = {"blob": "plane", "plane": "clusters", "lattice": "blob", "clusters": "lattice"}
SINGLE_SIZES = (N3, 150000)
SINGLE_PLACES = {"blob": ("local", "mm_local", "local1e6", "utm"), "plane": ("local", "mm_local"), "lattice": ("local", "mm_local", "local1e6", "utm"),
                 "clusters": ("local", "mm_local")}
N_OTHER, N_NEAR, N_BLOB = 900, 500, 200          # + 2 far queries = 1602 = 25 waves and 2 lanes


def _rng(*key):
    return np.random.Generator(np.random.PCG64(sum(map(ord, "".join(str(k) for k in key)))))


def random_cloud(rng, n, kind, scale=1.0):
    """tests/test_gpu_parity.py:_random_cloud for the four kinds used here (restated: that module cannot be imported without a GPU run)"""
    if kind == "blob":
        p = rng.normal(0.0, 0.05, (n, 3))
    elif kind == "plane":
        p = np.column_stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), np.zeros(n)])
    elif kind == "lattice":
        side = int(np.ceil(n ** 0.5))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64)
        p = np.column_stack([g * 0.0078125, np.full(n, 0.25)])
    elif kind == "clusters":
        p = np.vstack([rng.normal(-0.5, 0.01, (n // 2, 3)), rng.normal(0.5, 0.01, (n - n // 2, 3))])
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(p * scale)


def single_query_case(place, kind, n):
    """(target of n points, 1602 queries) of tests/test_gpu_nn_depth3.py a: the query mix of
    test_gpu_nn_offorigin.py:test_single_queries_every_kernel — another cloud's points, target points +- 1e-9 of the data scale, a blob,
    two far ones (1e3 extents and 1e6 m away) — with the near ones drawn from the whole target, so that they fall into every part of the tree."""
    rng = _rng(place, kind, n)
    s = oo.place_scale(place)
    dst = oo.place_points(place, random_cloud(rng, n, kind))
    other = oo.place_points(place, random_cloud(rng, N_OTHER, OTHER_KIND[kind]))
    pick = rng.choice(n, N_NEAR, replace=False)
    near = dst[pick] + rng.choice([-1e-9, 1e-9], (N_NEAR, 3)) * s
    blob = oo.place_points(place, random_cloud(rng, N_BLOB, "blob"))
    centre = dst.mean(0)
    extent = max(float(np.ptp(dst, axis=0).max()), s)
    far = np.array([centre + 1e3 * extent * np.array([0.6, -0.64, 0.48]), centre + np.array([0.0, 0.0, 1e6])])
    return dst, np.ascontiguousarray(np.vstack([other, near, blob, far]))


def ragged_target(n):
    """a blob of n points at the local site frame (n = RAGGED_SIZES: the last tile holds one point)"""
    return oo.place_points("local", random_cloud(_rng("ragged", n), n, "blob"))


def ragged_queries(dst, last_idx, n_rest=1200):
    """queries on the given target points (the last tile's) and +- 1e-9 beside them along every axis, next to n_rest queries across the
    rest of the cloud (target points +- 1e-9 and a blob).  -> (queries, number of queries that belong to the last tile's points)"""
    rng = _rng("ragged queries", len(dst))
    own = dst[np.asarray(last_idx)]
    step = np.vstack([np.zeros((1, 3)), 1e-9 * np.eye(3), -1e-9 * np.eye(3), 1e-9 * np.array([[1, 1, 1], [-1, -1, -1], [1, -1, 1]])])
    mine = (own[:, None, :] + step[None]).reshape(-1, 3)
    pick = rng.choice(len(dst), n_rest // 2, replace=False)
    rest = np.vstack([dst[pick] + rng.choice([-1e-9, 1e-9], (len(pick), 3)), oo.place_points("local", random_cloud(rng, n_rest - len(pick) + 3, "blob"))])
    return np.ascontiguousarray(np.vstack([mine, rest])), len(mine)


LATTICE_SHAPE = (363, 362)
LATTICE_H = 2.0 ** -7


def lattice_tie_case(n_each=300):
    """A 363 x 362 range-image lattice of spacing 2^-7 at z = 0.25 (131 406 points) and queries whose answer a tie rule decides:
    on lattice points (one target at distance 0), exactly between two x-neighbours and exactly in the middle of a cell, 0.1 .. 0.4
    spacings above the lattice (2 and 4 targets at exactly the same distance: every coordinate is a dyadic number, so the sums are exact),
    and within +- 3e-10 of the bisector plane between two x-neighbours as in offorigin.bisector_problem (no exact tie, a gap below a
    nanometre).  -> (target, queries, ties) with ties[j] = the target indices that must be at exactly the best distance of query j
    (() for the bisector queries)."""
    rng = _rng("lattice ties")
    a, b = LATTICE_SHAPE
    h = LATTICE_H
    g = np.stack(np.meshgrid(np.arange(a), np.arange(b), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    dst = np.ascontiguousarray(np.column_stack([g * h, np.full(len(g), 0.25)]))
    ix = rng.integers(0, a - 1, 4 * n_each); iy = rng.integers(0, b - 1, 4 * n_each)
    up = rng.integers(13, 52, 4 * n_each) * (h / 128)          # dyadic heights, 0.1 .. 0.4 h
    q, ties = [], []
    for j in range(4 * n_each):
        x, y, k = ix[j], iy[j], j // n_each
        if k == 0:
            q.append([x * h, y * h, 0.25]); ties.append((x * b + y,))
        elif k == 1:
            q.append([(x + 0.5) * h, y * h, 0.25 + up[j]]); ties.append((x * b + y, (x + 1) * b + y))
        elif k == 2:
            q.append([(x + 0.5) * h, (y + 0.5) * h, 0.25 + up[j]]); ties.append((x * b + y, x * b + y + 1, (x + 1) * b + y, (x + 1) * b + y + 1))
        else:
            q.append([(x + 0.5) * h + rng.uniform(-3e-10, 3e-10), y * h + rng.uniform(-0.2, 0.2) * h, 0.25 + rng.uniform(0.1, 0.4) * h]); ties.append(())
    return dst, np.ascontiguousarray(np.array(q)), ties


N_UNIQUE = 65537


def duplicate_case(n_each=400):
    """65 537 points of a blob, each stored twice at unrelated indices (131 074 points), and queries exactly on a pair (distance 0 twice),
    1e-4 beside a pair (the same positive distance twice) and elsewhere.  -> (target, queries)"""
    rng = _rng("duplicates")
    base = rng.normal(0.0, 0.05, (N_UNIQUE, 3))
    dst = np.ascontiguousarray(np.vstack([base, base[rng.permutation(N_UNIQUE)]]))
    pick = rng.choice(N_UNIQUE, 2 * n_each, replace=False)
    q = np.vstack([base[pick[:n_each]], base[pick[n_each:]] + 1e-4, rng.normal(0.0, 0.05, (n_each, 3))])
    return dst, np.ascontiguousarray(q)


def dist2(q, p):
    """nn_metric.h:dist2 on rows: (dx dx + dy dy) + dz dz"""
    d = np.asarray(q) - np.asarray(p)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


MIXED_SIZES = (N3, 3000, 500)


def mixed_case():
    """targets of 3, 2 and 1 box levels (131 073, 3000 and 500 points: a blob, a lattice, a plane, all at the local site frame) and one
    query set for all three"""
    rng = _rng("mixed")
    targets = [oo.place_points("local", random_cloud(rng, n, kind)) for n, kind in zip(MIXED_SIZES, ("blob", "lattice", "plane"))]
    pick = rng.choice(MIXED_SIZES[0], 400, replace=False)
    q = np.vstack([targets[0][pick] + rng.choice([-1e-9, 1e-9], (400, 3)), targets[1][:300] + 1e-9, targets[2][:200] - 1e-9,
                   oo.place_points("local", random_cloud(rng, 350, "blob")), oo.place_points("local", random_cloud(rng, 352, "plane"))])
    return targets, np.ascontiguousarray(q)


# ---- the cached rounds
ROUNDS_TARGET, ROUNDS_SOURCE = 140000, 4000
ROUNDS_MAGS = [3e-3, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7]
# The script for MVICP_NN_AUTO.  AUTO runs its cache-aware rounds only while the median distance of the last search is below 1.5 hash
# cells of the target (about 3 mm for 140 000 points on this surface); it is 0.43 mm at the ground truth, 2.8 mm after the 3e-3 move of
# the script above and 3.2 mm after its 1e-3 move, where AUTO goes back to the plain seeded build for good.  These moves leave 1.1 mm.
ROUNDS_MAGS_SETTLED = [1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 1e-6]
ROUNDS_CUTOFF = 0.05
ROUNDS_PLACES = ("unit", "mm_utm")


def rounds_problem():
    """Three views of the bumpy sphere (synth.make_view of a 3-view ring: normals exist): view 0 with 140 000 points is the target of
    both edges, views 1 and 2 with 4000 points each are the sources.  -> the dict of synth.make_problem"""
    pb = synth.make_poses(3)
    pts, nor = [], []
    for k, n in enumerate((ROUNDS_TARGET, ROUNDS_SOURCE, ROUNDS_SOURCE)):
        p, m = synth.make_view(k, 3, n)
        pts.append(p); nor.append(m)
    pb["pts"] = pts; pb["nor"] = nor
    pb["src"] = np.array([1, 2], dtype=np.int32); pb["dst"] = np.array([0, 0], dtype=np.int32)
    return pb


def placed_rounds(place, start="init"):
    """(problem, placed points, normals, the eight placed pose sets of offorigin.scripted_poses, the placed cutoff).  start = "init": the
    script ROUNDS_MAGS from the problem's noisy initial poses (a centimetre off: MVICP_NN_AUTO never hands over); "gt": the script
    ROUNDS_MAGS_SETTLED from the ground truth (a converged registration that still moves: AUTO hands over and runs its cache-aware rounds)."""
    pb = rounds_problem()
    seq = oo.scripted_poses(pb[start], ROUNDS_MAGS if start == "init" else ROUNDS_MAGS_SETTLED, 11)
    pts, nor, _, thresh, pl = oo.place(place, pb["pts"], pb["nor"], seq[0], ROUNDS_CUTOFF)
    return pb, pts, nor, [pl.poses(P) for P in seq], thresh
