"""The kernel paths that the host picks from the input sizes, and cases that reach each of them.  Test infrastructure only.

The dispatch constants are read from the project's sources by name (a name that is not found raises), and the host arithmetic of
csrc/consensus.hip:consensus() and csrc/match.hip:chunking() / launch_direction() is restated here as small pure functions of the sizes
and those constants.  A case states the path it is built for as a condition on the plan, so a constant that changes makes the case's
precondition fail instead of silently losing the coverage (tests/test_paths_cpu.py asserts every condition without a GPU;
tests/test_gpu_paths.py asserts it again next to the run).  Every case is seeded with PCG64 and every expensive reference is computed
once per process."""
import functools
import os
import re

import numpy as np

import matchref as mr
import offorigin
import outlierref
import voxelref
from mvicp import synth

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mv-lm-icp_amd", "csrc")
GRID_Y_MAX = 65535   # the HIP limit on gridDim.y (a literal in consensus(), kMaxChunks in match.hip)


# ---- the constants, from the sources
def read_source(name, csrc=None):
    with open(os.path.join(csrc or CSRC, name)) as f:
        return f.read()


def int_constants(text, names, where):
    """{name: value} of `constexpr int NAME = VALUE;`"""
    out = {}
    for name in names:
        found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % re.escape(name), text)
        if len(found) != 1:
            raise LookupError("%s: `constexpr int %s = ...;` found %d times" % (where, name, len(found)))
        out[name] = int(found[0])
    return out


def outlier_thresholds(text, where="csrc/outlier.hip"):
    """[(largest k, list capacity), ...] of outlier_filter's dispatch `k <= A -> <CA>`, `k <= B -> <CB>`, else `<CC>` (k <= CC - 1: the
    list holds the point itself and k neighbours), ascending."""
    body = text[text.index("long long outlier_filter("):] if "long long outlier_filter(" in text else ""
    arms = re.findall(r"if\s*\(k\s*<=\s*(\d+)\)\s*hipLaunchKernelGGL\(outlier_knn_kernel<(\d+)>", body)
    last = re.findall(r"else\s+hipLaunchKernelGGL\(outlier_knn_kernel<(\d+)>", body)
    if len(arms) != 2 or len(last) != 1:
        raise LookupError("%s: the dispatch `k <= A`, `k <= B`, else of outlier_filter not found (%d arms, %d else)" % (where, len(arms), len(last)))
    out = [(int(a), int(c)) for a, c in arms] + [(int(last[0]) - 1, int(last[0]))]
    if not all(out[i][0] < out[i + 1][0] for i in range(2)) or any(k + 1 > cap for k, cap in out):
        raise LookupError("%s: the thresholds %r do not ascend or exceed their capacity" % (where, out))
    return out


def load_constants(csrc=None):
    return {"consensus": int_constants(read_source("consensus.hip", csrc), ("kThreads", "kPairTile", "kWantBlocks"), "csrc/consensus.hip"),
            "match": int_constants(read_source("match.hip", csrc), ("kThreads", "kTile", "kGenRows", "kGenTile", "kMaxChunks"), "csrc/match.hip"),
            "outlier": outlier_thresholds(read_source("outlier.hip", csrc))}


CONSTANTS = load_constants()


def _cdiv(a, b):
    return -(-a // b)


# ---- the plans
def consensus_plan(n_pairs, n_acc, k=None):
    """The grid of cons_score_kernel for n_pairs pairs and n_acc accepted hypotheses (n_acc > 0), as consensus() computes it.
    -> dict(gx, gy, per_y, tiles, tiles_per_block, rows_in_last_block, tiles_in_last_block, rows_in_last_tile)"""
    k = k or CONSTANTS["consensus"]
    assert n_pairs > 0 and n_acc > 0
    gx = _cdiv(n_acc, k["kThreads"])
    tiles = _cdiv(n_pairs, k["kPairTile"])
    gy = min(_cdiv(k["kWantBlocks"], gx), tiles, GRID_Y_MAX)
    split = max(gy, 1)                  # (the split asked for; whole tiles per row can make the launched grid shorter)
    per_y = min(_cdiv(tiles, split) * k["kPairTile"], n_pairs)
    gy = _cdiv(n_pairs, per_y)          # (the launched one)
    last = n_pairs - (gy - 1) * per_y
    return {"gx": gx, "gy": gy, "split": split, "per_y": per_y, "tiles": tiles, "tiles_per_block": _cdiv(per_y, k["kPairTile"]), "rows_in_last_block": last,
            "tiles_in_last_block": _cdiv(last, k["kPairTile"]), "rows_in_last_tile": last - (_cdiv(last, k["kPairTile"]) - 1) * k["kPairTile"]}


def consensus_score_bytes(plan, n_pairs, n_acc):
    """the model bytes that consensus() books on the scope "cons_score" """
    return (48.0 * n_pairs) * plan["gx"] + 148.0 * n_acc


def consensus_gx_from_bytes(model_bytes, n_pairs, n_acc):
    return (model_bytes - 148.0 * n_acc) / (48.0 * n_pairs)


def match_plan(match_chunk, rows, right, dim, k=None):
    """One direction of feature_match: `rows` left rows against `right` rows of the other operand, as chunking() and launch_direction()
    compute it.  -> dict(chunk, chunks, clamped, tile, tiles_per_chunk, rows_in_last_tile (of a whole chunk), rows_in_last_chunk,
    tiles_in_last_chunk, rows_in_last_tile_of_last_chunk, wgs (workgroups of left rows))"""
    k = k or CONSTANTS["match"]
    assert rows > 0 and right > 0
    ch = match_chunk if match_chunk > 0 else 1
    clamped = _cdiv(right, ch) > k["kMaxChunks"]
    if clamped:
        ch = _cdiv(right, k["kMaxChunks"])
    if ch > right:
        ch = right
    chunks = _cdiv(right, ch)
    tile = k["kTile"] if dim == 33 else k["kGenTile"]
    left = k["kThreads"] if dim == 33 else k["kGenRows"]
    last = right - (chunks - 1) * ch
    return {"chunk": ch, "chunks": chunks, "clamped": clamped, "tile": tile, "tiles_per_chunk": _cdiv(ch, tile),
            "rows_in_last_tile": ch - (_cdiv(ch, tile) - 1) * tile, "rows_in_last_chunk": last, "tiles_in_last_chunk": _cdiv(last, tile),
            "rows_in_last_tile_of_last_chunk": last - (_cdiv(last, tile) - 1) * tile, "wgs": _cdiv(rows, left)}


def match_bytes(plan, rows, right, dim):
    """the model bytes that launch_direction() books on the scope "match_fwd" / "match_bwd" """
    return 8.0 * dim * (float(rows) * plan["chunks"] + float(plan["wgs"]) * right) + 24.0 * float(rows) * plan["chunks"]


def match_chunks_from_bytes(model_bytes, wgs, rows, right, dim):
    return (model_bytes - 8.0 * dim * float(wgs) * right) / ((8.0 * dim + 24.0) * rows)


def outlier_capacity(k, table=None):
    """the list capacity of outlier_knn_kernel that outlier_filter launches for k"""
    for kmax, cap in (table or CONSTANTS["outlier"]):
        if k <= kmax:
            return cap
    raise ValueError("k = %d is above every capacity" % k)


def outlier_boundary_ks(table=None):
    """1, both sides of every boundary between two capacities, the largest k"""
    t = table or CONSTANTS["outlier"]
    return (1, t[0][0], t[0][0] + 1, t[1][0], t[1][0] + 1, t[2][0])


OUTLIER_SWEEP_K = (1, 8, 9, 16, 17, 32)   # test_gpu_outlier.py:test_size_sweep; test_paths_cpu.py holds it against outlier_boundary_ks()


# ---- consensus
CONS_TAU, CONS_EDGE_SIM, CONS_SEED = 0.03, 0.0, 77
CONS_W, CONS_T = (0.3, -0.5, 0.8), (0.4, -0.1, 0.25)
CONS_SHAPES = {"C1": (262144 + 513, 16), "C2": (700, 140000), "C3": (3 * 256 + 1, 3000), "C4": (3 * 256 + 1, 3000)}


@functools.lru_cache(maxsize=None)
def consensus_pairs(name):
    """-> (P, Q, H): P uniform in the unit cube; Q = R P + t + N(0, 0.01), then every second row replaced by a uniform point of the
    cube moved the same way (an outlier).  "C4" is "C3" with offorigin.WU added to both (the rounding of the sums is part of the input)."""
    if name == "C4":
        P, Q, H = consensus_pairs("C3")
        return np.ascontiguousarray(P + offorigin.WU), np.ascontiguousarray(Q + offorigin.WU), H
    c, H = CONS_SHAPES[name]
    rng = np.random.Generator(np.random.PCG64(1000 + c))
    P = rng.uniform(0.0, 1.0, size=(c, 3))
    R = synth.so3_exp(np.array(CONS_W))
    Q = P @ R.T + np.array(CONS_T) + rng.normal(0.0, 0.01, size=(c, 3))
    out = rng.uniform(0.0, 1.0, size=(c, 3)) @ R.T + np.array(CONS_T)
    Q[1::2] = out[1::2]
    P, Q = np.ascontiguousarray(P), np.ascontiguousarray(Q)
    P.setflags(write=False); Q.setflags(write=False)
    return P, Q, H


@functools.lru_cache(maxsize=None)
def consensus_reference(name):
    P, Q, H = consensus_pairs(name)
    return mr.consensus(P, Q, H, CONS_SEED, CONS_TAU, CONS_EDGE_SIM)


def consensus_case_plan(name, k=None):
    P, _, _ = consensus_pairs(name)
    return consensus_plan(len(P), consensus_reference(name)["accepted"], k)


def check_consensus_case(name, k=None):
    """The conditions of the case on the plan and on the reference alone (AssertionError otherwise) -> (plan, reference)."""
    P, Q, H = consensus_pairs(name)
    c = len(P)
    want = consensus_reference(name)
    plan = consensus_case_plan(name, k)
    kk = k or CONSTANTS["consensus"]
    acc = want["counts"][want["counts"] >= 0]
    assert want["best"] >= 0 and 0 < want["count"] < c, (name, want["best"], want["count"])
    if name == "C1":     # many pairs, few hypotheses: every workgroup walks two tiles, the last one holds a single pair
        assert want["accepted"] >= 8 and len(np.unique(acc)) >= 8 and (acc < c).all(), (name, want["accepted"], np.unique(acc))
        assert plan["gx"] == 1 and plan["split"] == kk["kWantBlocks"] < plan["tiles"] == 1027 and plan["gy"] == 514, (name, plan)
        assert plan["tiles_per_block"] == 2 and plan["per_y"] == 2 * kk["kPairTile"] and plan["rows_in_last_block"] == 1, (name, plan)
    elif name == "C2":   # many accepted hypotheses: two workgroup rows, the first walks two tiles, the second one partial tile
        assert want["accepted"] >= 131073, (name, want["accepted"])
        assert plan["gx"] >= 513 and plan["gy"] == 2 and plan["gy"] < plan["tiles"] == 3, (name, plan)
        assert plan["tiles_per_block"] == 2 and plan["tiles_in_last_block"] == 1 and 1 < plan["rows_in_last_block"] < kk["kPairTile"], (name, plan)
    else:                # C3 / C4: one tile per workgroup row and a last row of one pair
        assert want["accepted"] > 2900, (name, want["accepted"])
        assert plan["gx"] > 1 and plan["tiles_per_block"] == 1 and plan["gy"] == plan["tiles"] == 4 and plan["rows_in_last_block"] == 1, (name, plan)
    if name == "C4":
        near = consensus_reference("C3")
        assert np.abs(P).max() > 4e6 and want["count"] >= 0.3 * near["count"], (name, np.abs(P).max(), want["count"], near["count"])
        # The rounding of the placed coordinates (half a nanometre) is part of the input: the winner's rotation differs in its low bits
        # and its translation, a difference of sums near 4e6, by more than that (the rotation's change times a lever of 4e6), so `pose`
        # tells an operation order apart.  The integer counts do NOT differ from the unplaced ones: a residual within a nanometre of
        # tau = 0.03 does not occur among these 2.3 million.
        assert want["best"] == near["best"] and want["pose"][:3, :3].tobytes() != near["pose"][:3, :3].tobytes()
        shifted = near["pose"][:3, 3] + offorigin.WU - near["pose"][:3, :3] @ offorigin.WU
        assert np.abs(want["pose"][:3, 3] - shifted).max() > 1e-9, np.abs(want["pose"][:3, 3] - shifted).max()
    return plan, want


# ---- matching
MATCH_DIMS = (33, 5)
MATCH_DEFAULT_CHUNK = 2048


def _frozen(*arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.float64)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def match_m1(dim):
    """3 x 70000 uniform descriptors: with match_chunk = 1 the forward direction would need 70000 chunks"""
    rng = np.random.Generator(np.random.PCG64(4100 + dim))
    return _frozen(rng.uniform(0.0, 100.0, size=(3, dim)), rng.uniform(0.0, 100.0, size=(70000, dim)))


@functools.lru_cache(maxsize=None)
def match_m2(dim):
    """300 x 257 small integers, the rows 128.. of b repeat its rows 0..: exact ties for the first and the second place"""
    rng = np.random.Generator(np.random.PCG64(4200 + dim))
    a = rng.integers(0, 3, size=(300, dim)).astype(np.float64)
    b = rng.integers(0, 3, size=(257, dim)).astype(np.float64)
    b[257 // 2:] = b[:257 - 257 // 2]
    return _frozen(a, b)


M2_CHUNK = 100
M3_FAR = 200


@functools.lru_cache(maxsize=None)
def match_m3(order):
    """dim 33.  a: rows 0..63 (wave 0) a tight cluster round x0 (noise 1e-3 per column), rows 64..127 (wave 1) the same except that row 81
    lies 100 away from x0 in the columns 22..32.  b: two rows near x0 (0.05 and 0.06 off in every column), 200 far rows (5 .. 15 off in
    the columns 0..10 for the orders "a" and "b", in the columns 11..21 for "c"; 1e-3 noise elsewhere) and one row nearer than both
    (0.02 off).  "a", "c": near, near, the far rows, the nearer one; "b": the far rows first, then near, near, nearer.  In "a" and "b" the
    last far row is also 100 off in the columns 22..32: the nearest row of row 81, which its lane loses if the wave skips without it."""
    rng = np.random.Generator(np.random.PCG64(4300))
    x0 = rng.uniform(0.0, 100.0, size=33)
    a = x0 + rng.normal(0.0, 1e-3, size=(128, 33))
    a[81, 22:33] += 100.0
    near = np.stack([x0 + 0.05, x0 + 0.06])
    nearer = (x0 + 0.02)[None]
    far = x0 + rng.normal(0.0, 1e-3, size=(M3_FAR, 33))
    cols = slice(11, 22) if order == "c" else slice(0, 11)
    far[:, cols] += rng.uniform(5.0, 15.0, size=(M3_FAR, 11)) * rng.choice([-1.0, 1.0], size=(M3_FAR, 11))
    if order != "c":
        far[-1, 22:33] += 100.0     # the last far row is the nearest of row 81, and of no other row
    b =np.concatenate([far, near, nearer]) if order == "b" else np.concatenate([near, far, nearer])
    return _frozen(a, b)


def m3_far_rows(order):
    return np.arange(0, M3_FAR) if order == "b" else np.arange(2, 2 + M3_FAR)


def partial_dist(a, b, cols):
    """the running sum of dist(a, b) after the first `cols` columns, for every pair -> (m, n)"""
    return mr.dist_matrix(a[:, :cols], b[:, :cols])


def running_second(D):
    """R[i, j] = the second smallest of D[i, :j] (+inf while fewer than two): the second best a lane holds when candidate j arrives"""
    m, n = D.shape
    R = np.full((m, n), np.inf)
    d0, d1 = np.full(m, np.inf), np.full(m, np.inf)
    for j in range(n):
        R[:, j] = d1
        d = D[:, j]
        first = d < d0
        second = ~first & (d < d1)
        d1 = np.where(first, d0, np.where(second, d, d1))
        d0 = np.where(first, d, d0)
    return R


@functools.lru_cache(maxsize=None)
def match_m4(dim):
    """130 x 257 uniform descriptors; the rows 5 and 100 of a and every 12th row of b (from row 3) scaled by 1e200: finite values whose
    squared differences overflow to +inf"""
    rng = np.random.Generator(np.random.PCG64(4400 + dim))
    a, b = rng.uniform(1.0, 100.0, size=(130, dim)), rng.uniform(1.0, 100.0, size=(257, dim))
    a[[5, 100]] *= 1e200
    b[3::12] *= 1e200
    return _frozen(a, b)


MATCH_BUILDERS = {"M1": match_m1, "M2": match_m2, "M3a": lambda dim: match_m3("a"), "M3b": lambda dim: match_m3("b"), "M3c": lambda dim: match_m3("c"),
                  "M4": match_m4}


@functools.lru_cache(maxsize=None)
def match_reference(name, dim):
    a, b = MATCH_BUILDERS[name](dim)
    with np.errstate(over="ignore"):
        return mr.feature_match(a, b)


def match_case_plans(name, dim, match_chunk, k=None):
    """-> (forward plan, backward plan)"""
    a, b = MATCH_BUILDERS[name](dim)
    return match_plan(match_chunk, len(a), len(b), dim, k), match_plan(match_chunk, len(b), len(a), dim, k)


def check_match_case(name, dim, match_chunk=MATCH_DEFAULT_CHUNK, k=None):
    """The conditions of the case on the plans and on the reference alone -> (forward plan, backward plan, reference)."""
    a, b = MATCH_BUILDERS[name](dim)
    want = match_reference(name, dim)
    fwd, bwd = match_case_plans(name, dim, match_chunk, k)
    kk = k or CONSTANTS["match"]
    if name == "M1":      # the clamp: more chunks asked for than a grid may have
        assert match_chunk == 1 and fwd["clamped"] and fwd["chunk"] == 2 and fwd["chunks"] == 35000 <= kk["kMaxChunks"], fwd
        assert not bwd["clamped"] and bwd["chunk"] == 1 and bwd["chunks"] == 3 and len(b) == 70000 and bwd["wgs"] > 1, bwd
    elif name == "M2":    # a chunk that ends inside a tile, with ties across the chunks
        assert match_chunk == M2_CHUNK
        for p in (fwd, bwd):
            assert p["chunks"] == 3 and p["chunk"] == M2_CHUNK and p["tiles_per_chunk"] >= 2 and 0 < p["rows_in_last_tile"] < p["tile"], p
        assert fwd["rows_in_last_chunk"] == 57 and 0 < fwd["rows_in_last_tile_of_last_chunk"] < fwd["tile"], fwd
        if dim == 33:
            assert fwd["wgs"] == 2 and (fwd["tiles_per_chunk"], fwd["rows_in_last_tile"]) == (2, 36), fwd
        else:
            assert (fwd["tiles_per_chunk"], fwd["rows_in_last_tile"]) == (4, 4), fwd
        tie = want["fwd_d2"][:, 0] == want["fwd_d2"][:, 1]
        assert tie.sum() > 60 and (want["fwd_idx"][tie, 0] < want["fwd_idx"][tie, 1]).all(), tie.sum()
        assert (want["fwd_idx"][tie, 0] // fwd["chunk"] != want["fwd_idx"][tie, 1] // fwd["chunk"]).sum() > 30
        tie = want["bwd_d2"][:, 0] == want["bwd_d2"][:, 1]
        assert tie.sum() > 10
    elif name.startswith("M3"):
        assert dim == 33 and fwd["chunks"] == 1 and fwd["wgs"] == 1 and len(a) == 128
        order = name[2]
        D = mr.dist_matrix(a, b)
        p11, p22 = partial_dist(a, b, 11), partial_dist(a, b, 22)
        run, final = running_second(D), want["fwd_d2"][:, 1]
        far = m3_far_rows(order)
        w0, w1, odd = np.arange(0, 64), np.arange(64, 128), 81
        assert np.isfinite(final).all()
        if order == "a":
            # wave 0: every lane is past its second best after the first segment, for every far row (the running second best is
            # what the lane holds then; the final one is the smallest it ever holds)
            assert (p11[np.ix_(w0, far)] > final[w0, None]).all() and (p11[np.ix_(w0, far)] > run[np.ix_(w0, far)]).all()
            # wave 1: 63 lanes are past it, the odd row is not, neither after the first nor after the second segment
            others = w1[w1 != odd]
            assert (p11[np.ix_(others, far)] > run[np.ix_(others, far)]).all()
            assert (p11[odd, far] <= final[odd]).all() and (p22[odd, far] <= run[odd, far]).all()
            assert (want["fwd_idx"][w0] == [len(b) - 1, 0]).all()        # the row that arrives last is the nearest
            assert want["fwd_idx"][odd, 0] == far[-1]                     # the odd row's nearest is a far row: a wave that skipped it loses it
        elif order == "b":
            # the far rows arrive while the slots are empty or hold far rows (some skipped, some not); the three near rows arrive last
            # and must enter
            assert (want["fwd_idx"][w0] == [len(b) - 1, len(b) - 3]).all()
            skip = (p11[np.ix_(w0, far)] > run[np.ix_(w0, far)]).all(0)
            assert not skip[:2].any() and skip[2:].any() and not skip[2:].all()
        else:
            # wave 0: not past the second best after the first segment, past it after the second
            assert (p11[np.ix_(w0, far)] <= final[w0, None]).all() and (p11[np.ix_(w0, far)] <= run[np.ix_(w0, far)]).all()
            assert (p22[np.ix_(w0, far)] > final[w0, None]).all() and (p22[np.ix_(w0, far)] > run[np.ix_(w0, far)]).all()
            assert (want["fwd_idx"][w0] == [len(b) - 1, 0]).all()
    elif name == "M4":
        for key in mr.MATCH_KEYS:
            assert not np.isnan(want[key].astype(np.float64)).any(), key
        both_f = np.isinf(want["fwd_d2"]).all(1)
        both_b = np.isinf(want["bwd_d2"]).all(1)
        assert both_f.sum() >= 1 and both_b.sum() > 10, (both_f.sum(), both_b.sum())
        assert (want["fwd_idx"][both_f] == [0, 1]).all() and (want["bwd_idx"][both_b] == [0, 1]).all()
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert (~both_f).sum() > 100 and np.isfinite(want["fwd_d2"][~both_f]).all()     # the other rows are ordinary
    return fwd, bwd, want


# ---- the outlier filter far from the origin
O1_PARAMS = ((8, 2.0, 0.0), (16, 1.0, 0.08e-3), (17, -1.0, 0.08e-3))


@functools.lru_cache(maxsize=None)
def outlier_far_cloud():
    """outlierref.sheet_cloud(2000, 7) in millimetres at a local site frame, then at UTM coordinates -> (points, normals)"""
    p, nr, _ = outlierref.sheet_cloud(2000, 7)
    q = offorigin.place_points("mm_local", p, shift_extra=offorigin.WU)
    return _frozen(q, nr)


@functools.lru_cache(maxsize=None)
def outlier_far_reference(k, std_ratio, radius):
    p, nr = outlier_far_cloud()
    return outlierref.outlier_filter(p, nr, k, std_ratio, radius)


def check_outlier_far(k, std_ratio, radius):
    p, _ = outlier_far_cloud()
    want = outlier_far_reference(k, std_ratio, radius)
    n, kept = len(p), want["stats"]["kept"]
    assert np.abs(p).max() > 4e6 and (p.max(0) - p.min(0)).max() < 2e-3, (np.abs(p).max(), p.max(0) - p.min(0))
    assert 0.9 * n < kept < n, kept
    return want


# ---- the voxel grid
V1_SHIFT, V1_SHIFT_WIDER, V1_SHIFT_REFUSED = 500.0, 600.0, 900.0
V1_VOXELS = (1e-3, 2.0 ** -10)


@functools.lru_cache(maxsize=None)
def voxel_two_clusters(shift):
    """two clusters of 2500 points, each uniform in a cube of edge 0.01, at (-shift, -shift, -shift) and (+shift, +shift, +shift),
    shuffled together, with unit normals -> (points, normals)"""
    rng = np.random.Generator(np.random.PCG64(5100))
    p = rng.uniform(0.0, 0.01, size=(5000, 3))
    p[:2500] -= shift
    p[2500:] += shift
    nr = rng.normal(size=(5000, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    perm = rng.permutation(5000)
    return _frozen(p[perm], nr[perm])


def voxel_key_bits(W, h):
    """-> (bits of the sort key, as voxel_reduce() chooses them; the number of cells)"""
    Cc = voxelref.cells(W, h)
    d = Cc.max(axis=0) - Cc.min(axis=0) + 1
    total = int(d[0]) * int(d[1]) * int(d[2])
    bits = 1
    while bits < 62 and (1 << bits) < total:
        bits += 1
    return bits, total


@functools.lru_cache(maxsize=None)
def voxel_v1_reference(shift, h):
    p, nr = voxel_two_clusters(shift)
    return voxelref.voxel_grid([p], [nr], h)


def check_voxel_v1(shift, h):
    p, nr = voxel_two_clusters(shift)
    bits, total = voxel_key_bits(p, h)
    want = voxel_v1_reference(shift, h)
    assert 58 <= bits <= 61 and total < 2 ** 62, (bits, total)
    assert (want["cnt"] > 1).sum() > 300 and (p < -shift / 2).all(1).sum() == 2500
    return bits, want


V2_VOXEL, V2_VOXEL_REFUSED = 0.01, 0.001


@functools.lru_cache(maxsize=None)
def voxel_v2_problem():
    """synth.make_problem(3, 3000) at UTM coordinates -> (pts, nor, poses)"""
    pb = synth.make_problem(3, 3000)
    pts, nor, poses, _, _ = offorigin.place("utm", pb["pts"], pb["nor"], pb["init"], 0.05)
    return pts, nor, poses


@functools.lru_cache(maxsize=None)
def voxel_v2_reference():
    pts, nor, poses = voxel_v2_problem()
    return voxelref.voxel_grid(pts, nor, V2_VOXEL, None, poses)


def check_voxel_v2():
    pts, nor, poses = voxel_v2_problem()
    W, _, _ = voxelref.world(pts, nor, None, poses)
    want = voxel_v2_reference()
    assert np.abs(W / V2_VOXEL).max() > 4e8 and (want["cnt"] > 1).sum() > 1000, (np.abs(W / V2_VOXEL).max(), (want["cnt"] > 1).sum())
    try:
        voxelref.voxel_grid(pts, nor, V2_VOXEL_REFUSED, None, poses)
    except ValueError as ex:
        assert "2^31" in str(ex)
    else:
        raise AssertionError("the reference accepts a millimetre voxel at UTM coordinates")
    return want
