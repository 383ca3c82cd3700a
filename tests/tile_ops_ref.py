"""Host side of tests/test_gpu_tile_ops.py: seeded input generators and NumPy
restatements of the structural tile operations, the radix sort's pass rule, DimApply
and the multiway merge.  tests/test_tile_ops_cpu.py checks every one of them against
a brute-force dense computation, so that a machine without a GPU keeps them honest.

Tiles are the plain dicts of tests/helpers.py (DCSC: cp int64, jc/ir int32, val f64).
"""
import numpy as np

from helpers import DBL_MAX, INF, dcsc_from_cols, tile_cols

# --------------------------------------------------------------------------
# the radix sort's pass rule (csrc/cbg_internal.h low_bits, csrc/cbg_sort.hip)
# --------------------------------------------------------------------------
SORT_TILE = 4096   # csrc/cbg_sort.hip RS_TILE
SCAN_TILE = 2048   # csrc/cbg_tile.hip SCAN_TILE


def low_bits(maxval):
    """mask of the bits of values in [0, maxval] (csrc/cbg_internal.h low_bits)"""
    m = 0
    while maxval > m:
        m = (m << 1) | 1
    return m


def digit_passes(major_ext, minor_ext):
    """8-bit digit passes radix_sort_pairs makes over (major << 32 | minor) keys with
    major in [0, major_ext) and minor in [0, minor_ext): the non-zero bytes of the mask"""
    varying = (low_bits(major_ext - 1) << 32) | low_bits(minor_ext - 1)
    return sum(1 for shift in range(0, 64, 8) if (varying >> shift) & 0xFF)


def transpose_passes(m, n):
    """passes of Tile.transpose on an m x n tile: keys (row << 32 | col)"""
    return digit_passes(m, n)


NNZ_EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)
NNZ_EDGE_SHAPE = (300, 70000)     # 2 + 3 digit passes: odd
HUGE = (1 << 31) - 2              # the largest local dimension the C ABI takes
# (m, n) -> digit passes, nnz 9000 (capped at m * n); every count 1..8 occurs
PASS_SHAPES = (((1, 200), 1), ((200, 1), 1), ((200, 200), 2), ((1, 70000), 3), ((600, 600), 4), ((70000, 70000), 6),
               (((1 << 24) + 5, 3), 5), ((HUGE, 70000), 7), ((HUGE, HUGE), 8))
PASS_NNZ = 9000


# --------------------------------------------------------------------------
# generators
# --------------------------------------------------------------------------
def tile_from_triples(m, n, rows, cols, vals):
    """distinct (row, col) triples -> DCSC dict"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    o = np.lexsort((rows, cols))
    r, c, v = rows[o], cols[o], np.asarray(vals, np.float64)[o]
    jc, start = np.unique(c, return_index=True)
    return dict(m=int(m), n=int(n), cp=np.append(start, len(r)).astype(np.int64), jc=jc.astype(np.int32),
                ir=r.astype(np.int32), val=v)


def random_tile(rng, m, n, nnz, corners=False):
    """min(nnz, m * n) distinct uniformly drawn positions of an m x n tile with distinct
    values (a misplaced value then shows); corners: (m-1, n-1), (0, n-1) and (m-1, 0) are
    among them, so that the top row and column ids are present"""
    cells = m * n
    nnz = min(nnz, cells)
    must = sorted({(m - 1) * n + (n - 1), n - 1, (m - 1) * n}) if corners else []
    must = np.array(must[:nnz], np.int64)
    if cells <= 1 << 24:
        keys = rng.permutation(cells)[:nnz]
    else:
        keys = np.unique(rng.integers(0, cells, 2 * nnz + 16))
        keys = rng.permutation(keys)[:nnz]
        assert len(keys) == nnz
    if len(must):
        keys = np.concatenate([must, keys[~np.isin(keys, must)]])[:nnz]
    vals = (rng.permutation(nnz) + 1.0) * (1.0 / 1024) - 3.0
    return tile_from_triples(m, n, keys // n, keys % n, vals)


def cols_tile(rng, m, n, lens, ids=None, lo=0, hi=None, vals=None):
    """DCSC dict whose stored columns have the given lengths, at random ids with gaps (or
    at `ids`), each holding distinct ascending random rows of [lo, hi); distinct values"""
    hi = m if hi is None else hi
    ids = np.sort(rng.choice(n, len(lens), replace=False)) if ids is None else np.asarray(ids)
    cols = [np.zeros(0, np.int64)] * n
    for j, L in zip(ids, lens):
        cols[int(j)] = lo + np.sort(rng.choice(hi - lo, int(L), replace=False))
    nnz = int(np.sum(lens))
    return dcsc_from_cols(m, n, cols, (rng.permutation(nnz) + 1.0) * (1.0 / 1024) - 1.0 if vals is None else vals)


def one_row_tile(rng, m, n, row, nnz):
    """every entry in one row: nnz single-entry columns"""
    cols = np.sort(rng.choice(n, nnz, replace=False))
    return tile_from_triples(m, n, np.full(nnz, row), cols, rng.permutation(nnz) + 0.5)


def one_col_tile(rng, m, n, col, nnz):
    rows = np.sort(rng.choice(m, nnz, replace=False))
    return tile_from_triples(m, n, rows, np.full(nnz, col), rng.permutation(nnz) + 0.5)


def single_entry_cols_tile(rng, m, n, nzc):
    """nzc columns of one entry each among n > nzc column ids (gaps), random rows"""
    assert n > nzc
    cols = np.sort(rng.choice(n, nzc, replace=False))
    return tile_from_triples(m, n, rng.integers(0, m, nzc), cols, rng.permutation(nzc) + 0.25)


def regular_tile(rng, m, n, nnz):
    """nnz entries laid out without a sort: the columns 0..n-1 take nnz // n entries each
    (the first nnz % n one more), column j a run of consecutive rows starting at a
    column-dependent offset; the values are a seeded permutation of 1..nnz"""
    per, extra = divmod(nnz, n)
    cnt = np.full(n, per, np.int64)
    cnt[:extra] += 1
    assert cnt.max() <= m and cnt.min() >= 1
    cp = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    start = (np.arange(n, dtype=np.int64) * 7) % (m - cnt + 1)
    ir = np.arange(nnz, dtype=np.int64) - np.repeat(cp[:-1], cnt) + np.repeat(start, cnt)
    return dict(m=m, n=n, cp=cp, jc=np.arange(n, dtype=np.int32), ir=ir.astype(np.int32),
                val=rng.permutation(nnz).astype(np.float64) + 1.0)


def empty_tile(m, n):
    return dict(m=m, n=n, cp=np.zeros(1, np.int64), jc=np.zeros(0, np.int32), ir=np.zeros(0, np.int32),
                val=np.zeros(0, np.float64))


# --------------------------------------------------------------------------
# the restriction operator's draws (helpers.restriction_host, csrc/cbg_ops.hip)
# --------------------------------------------------------------------------
def restriction_row_draws(scale, seed=0x5EED):
    """entries drawn per fine row: the Poisson(1) count of helpers.restriction_host"""
    from helpers import POISSON1_CDF, _mix_np
    i = np.arange(1 << scale, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _mix_np(np.uint64(seed) ^ (i * np.uint64(0xD1B54A32D192ED03)))
        u = (_mix_np(h ^ np.uint64(0x5851F42D4C957F2D)) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.searchsorted(POISSON1_CDF, u, side="right")


# --------------------------------------------------------------------------
# DimApply (SpParMat.cpp:801, Operations.h:153-179)
# --------------------------------------------------------------------------
PALETTE = np.array([0.0, -0.0, 1.5, -1.5, INF, -INF, np.nan, 5e-324, DBL_MAX], np.float64)
DIM_LENS = (1, 64, 65, 200)
COLUMN, ROW = 0, 1


def dim_apply_case(seed=17):
    """(tile, vec_col, vec_row): len(PALETTE) groups of columns with the lengths DIM_LENS;
    the columns of group g meet the scaler PALETTE[g] under Column, row r meets
    PALETTE[r % 9] under Row, and the value at row r is PALETTE[(r // 9) % 9]: a column of
    64 or more entries holds every value, and rows r, r + 9, ... every (value, scaler) pair"""
    rng = np.random.default_rng(seed)
    P = len(PALETTE)
    m, n = 405, 2 * P * len(DIM_LENS)
    ids = np.sort(rng.choice(n, P * len(DIM_LENS), replace=False))
    t = cols_tile(rng, m, n, DIM_LENS * P, ids=ids)
    t["val"] = PALETTE[(t["ir"].astype(np.int64) // P) % P]
    vec_col = np.full(n, 7.25)            # columns that hold nothing: never read
    vec_col[ids] = PALETTE[np.arange(len(ids)) // len(DIM_LENS)]
    vec_row = PALETTE[np.arange(m) % P]
    return t, vec_col, vec_row


def dim_scalers(t, dim, vec):
    return np.asarray(vec, np.float64)[tile_cols(t) if dim == COLUMN else t["ir"].astype(np.int64)]


def palette_pairs(t, dim, vec):
    """the set of (value bits, scaler bits) pairs that meet in DimApply(dim, vec)"""
    v = np.ascontiguousarray(t["val"]).view(np.uint64)
    s = np.ascontiguousarray(dim_scalers(t, dim, vec)).view(np.uint64)
    return set(zip(v.tolist(), s.tolist()))


def dim_apply_host(t, dim, vec, op):
    """the reference's DimApply: op(value, scaler) with multiplies, plus, and
    minimum(x, y) = x < y ? x : y, maximum(x, y) = x < y ? y : x (Operations.h:153-179)"""
    v, s = t["val"], dim_scalers(t, dim, vec)
    with np.errstate(invalid="ignore", over="ignore"):
        out = {"multiplies": lambda: v * s, "plus": lambda: v + s, "min": lambda: np.where(v < s, v, s),
               "max": lambda: np.where(v < s, s, v)}[op]()
    return dict(t, val=out)


# --------------------------------------------------------------------------
# multiway merge (Friends.h:657-741)
# --------------------------------------------------------------------------
def merge_host(parts, sr):
    """MergeAll on host tiles of one shape: a stable sort of the parts' entries, laid end
    to end in part order, by (col, row); every run of equal keys folded in that order with
    a + b (plus) or std::min(a, b) = b < a ? b : a (minplus)"""
    m, n = parts[0]["m"], parts[0]["n"]
    key = np.concatenate([tile_cols(p) * m + p["ir"].astype(np.int64) for p in parts])
    val = np.concatenate([p["val"] for p in parts])
    if len(key) == 0:
        return empty_tile(m, n)
    o = np.argsort(key, kind="stable")
    key, val = key[o], val[o]
    head = np.ones(len(key), bool)
    head[1:] = key[1:] != key[:-1]
    run = np.cumsum(head) - 1
    first = np.flatnonzero(head)
    rank = np.arange(len(key)) - first[run]
    acc = val[first].copy()
    for k in range(1, int(rank.max()) + 1):
        at = np.flatnonzero(rank == k)
        a, b = acc[run[at]], val[at]
        acc[run[at]] = a + b if sr == "plus" else np.where(b < a, b, a)
    ukey = key[first]
    return tile_from_triples(m, n, ukey % m, ukey // m, acc)


def merge_parts(P, sr, seed=23, m=700, n=60):
    """P host partials of one shape.  In turn: a base part (columns of 1, 63, 64, 65, 130
    and 300 entries on even column ids), a part that shares some rows of the base's columns
    and adds rows of its own, an empty part, a part on odd column ids (disjoint columns),
    and a part that overlaps the base in every entry; then the same kinds again.
    plus: multiples of 2^-10 with both zeros, so every sum is exact in any order.
    minplus: a position held by ONE part carries -0.0, +0.0, +inf, DBL_MAX, -DBL_MAX or a
    subnormal (handed through unchanged); shared positions carry distinct non-zero finite
    values or +inf, so that the minimum does not depend on the order."""
    rng = np.random.default_rng(seed)
    lens = [1, 63, 64, 65, 130, 300, 1, 7, 64, 200]
    even = np.arange(0, n, 2)
    base_ids = np.sort(rng.choice(even, len(lens), replace=False))
    base = cols_tile(rng, m, n, lens, ids=base_ids)
    parts = []
    for p in range(P):
        kind = p % 5
        if kind in (0, 4):
            t = dict(base)
        elif kind == 2:
            t = empty_tile(m, n)
        elif kind == 3:
            t = cols_tile(rng, m, n, [1, 64, 129, 20], ids=np.sort(rng.choice(np.arange(1, n, 2), 4, replace=False)))
        else:
            cols = [np.zeros(0, np.int64)] * n
            for i, j in enumerate(base["jc"]):
                own = base["ir"][base["cp"][i]:base["cp"][i + 1]].astype(np.int64)
                keep = own[rng.random(len(own)) < 0.5]
                cols[int(j)] = np.union1d(keep, rng.choice(m, 1 + len(own) // 3, replace=False))
            t = dcsc_from_cols(m, n, cols)
        parts.append(t)
    key = np.concatenate([tile_cols(p) * m + p["ir"].astype(np.int64) for p in parts])
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    lone = cnt[inv] == 1
    if sr == "plus":
        val = rng.integers(-2048, 2048, len(key)).astype(np.float64) / 1024.0
        val[rng.random(len(key)) < 0.05] = -0.0
        val[rng.random(len(key)) < 0.05] = 0.0
    else:
        val = rng.permutation(len(key)) * 0.5 - 0.25 * len(key) + 0.25    # distinct, finite, never zero
        val[~lone & (rng.random(len(key)) < 0.1)] = INF
        special = np.array([-0.0, 0.0, INF, DBL_MAX, -DBL_MAX, 2.0 ** -1070])[rng.integers(0, 6, len(key))]
        val = np.where(lone & (rng.random(len(key)) < 0.5), special, val)
    out, e = [], 0
    for p in parts:
        k = len(p["ir"])
        out.append(dict(p, val=val[e:e + k].copy()))
        e += k
    return out


# --------------------------------------------------------------------------
# tiles of the split / concat / slice cases
# --------------------------------------------------------------------------
SPLIT_LENS = (1, 63, 64, 65, 130)


def split_case(seed=31, m=400, n=40):
    """a tile with gaps in jc, column lengths SPLIT_LENS twice over, rows inside [5, m - 5)
    (so that a row cut can send every entry to either side), and a column id that is
    followed by a gap"""
    rng = np.random.default_rng(seed)
    ids = np.array([2, 3, 7, 11, 12, 19, 25, 26, 33, 37])
    return cols_tile(rng, m, n, SPLIT_LENS * 2, ids=ids, lo=5, hi=m - 5)


def single_col_case(seed=32, m=400, n=40):
    rng = np.random.default_rng(seed)
    return cols_tile(rng, m, n, [70], ids=[17], lo=5, hi=m - 5)


REBUILD_SLOTS = (1, 4, 5, SCAN_TILE, SCAN_TILE + 1)   # stored columns: one wave, a 256-thread block of four
# waves and one more, the slot scan's one tile and its second level (csrc/cbg_rebuild.h)


def rebuild_case(nzc, seed=41, m=600):
    """nzc stored columns at ids with gaps: the first of length 1 with its row in [5, 200), the
    last (nzc > 1) of length 65 in [400, 595), the ones between in [200, 400) with the
    lengths SPLIT_LENS, then 1 or 2.  A row cut at 200 or 400 empties exactly the first or
    the last column on one side and every other column on the other."""
    rng = np.random.default_rng(seed + nzc)
    n = 2 * nzc + 3
    ids = np.sort(rng.choice(n, nzc, replace=False))
    mid = [SPLIT_LENS[i] if i < len(SPLIT_LENS) else 1 + i % 2 for i in range(max(nzc - 2, 0))]
    lens = ([1] + mid + [65])[:nzc] if nzc > 1 else [1]
    cols = [np.zeros(0, np.int64)] * n
    for p, (j, L) in enumerate(zip(ids, lens)):
        lo = 5 if p == 0 else 400 if p == nzc - 1 else 200
        cols[int(j)] = lo + np.sort(rng.choice(195, int(L), replace=False))
    nnz = int(np.sum(lens))
    return dcsc_from_cols(m, n, cols, (rng.permutation(nnz) + 1.0) * (1.0 / 1024) - 1.0)


def block_case(seed=33, m=23, n=19, nnz=30):
    return random_tile(np.random.default_rng(seed), m, n, nnz)


# --------------------------------------------------------------------------
# the digest's unsorted count (include/cbg.h cbg_tile_digest)
# --------------------------------------------------------------------------
def unsorted_host(t):
    """the count include/cbg.h documents, entry by entry: a row id not strictly above its
    predecessor in its column, a column id not strictly above the previous one, an empty
    column, cp[0] != 0, cp[nzc] != nnz"""
    cp, jc, ir = [int(x) for x in t["cp"]], [int(x) for x in t["jc"]], [int(x) for x in t["ir"]]
    bad = int(cp[0] != 0) + int(cp[-1] != len(ir))
    for i in range(len(jc)):
        bad += cp[i + 1] <= cp[i]
        bad += i > 0 and jc[i - 1] >= jc[i]
        bad += sum(1 for q in range(cp[i] + 1, cp[i + 1]) if ir[q - 1] >= ir[q])
    return int(bad)


def digest_base():
    """6 columns at ids with gaps; lengths 3, 130, 2, 64, 1, 5; dyadic values (vsum exact)"""
    rng = np.random.default_rng(61)
    d = cols_tile(rng, 500, 30, [3, 130, 2, 64, 1, 5], ids=[1, 4, 5, 11, 20, 28])
    d["val"] = rng.integers(-4096, 4096, len(d["ir"])).astype(np.float64) / 1024.0
    return d


def digest_variants():
    """(name, tile, documented count).  Malformed by ORDER only: cp stays non-decreasing
    inside [0, nnz] and every id inside the tile, so the kernel reads nothing out of bounds."""
    b = digest_base()
    nnz, nzc = len(b["ir"]), len(b["jc"])
    a1 = int(b["cp"][1])   # the 130-entry column

    def var(**kw):
        t = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in b.items()}
        for k, f in kw.items():
            f(t[k])
        return t

    def swap(i, j):
        def f(x):
            x[i], x[j] = x[j], x[i]
        return f

    def put(i, v):
        def f(x):
            x[i] = v
        return f

    out = [("valid", var(), 0),
           ("rows_swapped", var(ir=swap(a1 + 10, a1 + 11)), 1),
           ("rows_equal", var(ir=put(a1 + 21, int(b["ir"][a1 + 20]))), 1),
           ("rows_swapped_63_64", var(ir=swap(a1 + 63, a1 + 64)), 1),   # the pair spans two lane rounds
           ("rows_swapped_64_65", var(ir=swap(a1 + 64, a1 + 65)), 1),
           ("jc_swapped", var(jc=swap(2, 3)), 1),
           ("jc_equal", var(jc=put(3, int(b["jc"][2]))), 1),
           # cp[0] = 1: entry 0 belongs to no column, the first column keeps 2 ascending rows
           ("cp0_is_1", var(cp=put(0, 1)), 1),
           # cp[nzc] = nnz - 1: the last column keeps 4 ascending rows
           ("cp_end_short", var(cp=put(nzc, nnz - 1)), 1),
           ("two_violations", var(ir=swap(a1 + 10, a1 + 11), jc=put(3, int(b["jc"][2]))), 2),
           ("three_violations", var(ir=swap(a1 + 64, a1 + 65), jc=swap(2, 3), cp=put(0, 1)), 3)]
    # one empty column: a stored id in a gap whose cp step is 0
    e = var()
    e["jc"] = np.insert(e["jc"], 3, 8).astype(np.int32)
    e["cp"] = np.insert(e["cp"], 3, e["cp"][3]).astype(np.int64)
    out.append(("empty_column", e, 1))
    for name, t, _ in out:
        assert np.all(np.diff(t["cp"]) >= 0) and t["cp"][0] >= 0 and t["cp"][-1] <= len(t["ir"]), name
        assert t["ir"].min() >= 0 and t["ir"].max() < t["m"] and t["jc"].min() >= 0 and t["jc"].max() < t["n"], name
        assert len(t["cp"]) == len(t["jc"]) + 1 <= t["n"] + 1 and len(t["ir"]) == len(t["val"]) == nnz, name
    return out


# --------------------------------------------------------------------------
# pairs of tiles for Tile.equal: equal m, n, nnz, nzc, one structural entry apart
# --------------------------------------------------------------------------
def equal_cases():
    """(base, [(label, other)]), (one, [(label, other)]).  base: columns 2, 5, 9, 14 whose
    rows lie below the next column's rows, so that moving a cp boundary by one leaves a
    valid tile; others: one jc entry or one interior cp entry changed (first, middle,
    last).  one: 300 single-entry columns (nnz = nzc < nzc + 1); others: the last jc entry
    changed, and cp[nzc] = nnz - 1 -- the only way index nzc can differ; that tile is not
    a valid one, but k_tile_diff reads the arrays element by element only."""
    base = dcsc_from_cols(40, 20, [[]] * 2 + [[1, 2, 3]] + [[]] * 2 + [[5, 6, 7]] + [[]] * 3 + [[9, 10, 11]] +
                          [[]] * 4 + [[13, 14, 15]] + [[]] * 5, np.arange(12) + 1.0)
    others = []
    for i, newid in ((0, 1), (1, 6), (2, 10), (3, 19)):
        jc = base["jc"].copy()
        jc[i] = newid
        others.append((f"jc[{i}]", dict(base, jc=jc)))
    for i in (1, 2, 3):
        for step in (1, -1):
            cp = base["cp"].copy()
            cp[i] += step
            others.append((f"cp[{i}]{step:+d}", dict(base, cp=cp)))
    k = 300
    one = single_entry_cols_tile(np.random.default_rng(71), 50, 400, k)
    free = np.setdiff1d(np.arange(int(one["jc"][-2]) + 1, 400), one["jc"])
    jc = one["jc"].copy()
    jc[-1] = free[-1]
    cp = one["cp"].copy()
    cp[k] = k - 1
    return (base, others), (one, [("jc[last]", dict(one, jc=jc)), ("cp[nzc]", dict(one, cp=cp))])


# --------------------------------------------------------------------------
# dense brute force (tests/test_tile_ops_cpu.py)
# --------------------------------------------------------------------------
def to_dense(t):
    """(held mask, values) of a small tile"""
    held = np.zeros((t["m"], t["n"]), bool)
    vals = np.zeros((t["m"], t["n"]))
    c, r = tile_cols(t), t["ir"].astype(np.int64)
    assert not held[r, c].any() and len(np.unique(c * t["m"] + r)) == len(r)
    held[r, c] = True
    vals[r, c] = t["val"]
    return held, vals


def from_dense(held, vals):
    cols, rows = np.nonzero(held.T)
    return tile_from_triples(held.shape[0], held.shape[1], rows, cols, vals[rows, cols])
