"""Bitmap slabs under exact int32 accumulation (IACC; csrc/cbg_local.hip SlabLds, k_num_slab):
6 B of LDS per nonzero -- an int32 sum and the low 16 bits of the row above the slab's first
row, the top two bits rebuilt from the rank scan's prefixes -- and with them larger caps for
both launch classes; the f64-valued slabs keep 8 B per nonzero and their caps.  The symbolic
plans a pair's slabs against the large IACC cap where the multiply's verdict, decided on the
device before it runs, says IACC (SymPanelArgs::iacc_dev).

A has one row panel (m = 2^18).  Every B column holds two entries: an A column of N distinct
rows and a second A column over a subset of those rows, so the (column, panel) pair has more
than 4096 products (a bitmap-mode pair), exactly N nonzeros, and sums of two products.  C is
compared with oracle_local by bits (integers and half-integers: exact in any order); the route
is read from last_work_stats() and set against predict_slabs(), the symbolic's plan on the CPU.
The caps come from cbg.local_slab_caps()."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from helpers import abs_tile, assert_digest_eq, assert_tiles_bits_equal, assert_tiles_equal, golden, oracle_local
from test_gpu_aprep_cache import _grid, _mat, _phased

pytestmark = pytest.mark.gpu

PANEL = 1 << 18
FINE = 1 << 13          # csrc/cbg_local.hip FINE_LOG: a slab is a run of whole fine ranges
F64_SMALL, F64_LARGE = 3056, 12032
EXTRA = 2000            # rows of the second A column: N + EXTRA > 4096 products for every N here
BITMAP = ("bitmap_small_kept", "bitmap_small_mark", "bitmap_large_kept", "bitmap_large_mark")
ENV = ("CBG_STAGE_RUNS", "CBG_STAGE_RUNS_CAP", "CBG_BIG_FLOPS", "CBG_CUTS_CAP", "CBG_THIN", "CBG_BITMAP_BUDGET_GB")


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def predict_slabs(rows, large_cap):
    """nonzeros of the slabs the symbolic cuts a pair of these (distinct, one-panel) rows
    into: one slab when the pair fits large_cap, else consecutive nonempty fine ranges
    grouped greedily while a slab holds <= large_cap"""
    per = np.bincount(np.asarray(rows) // FINE, minlength=PANEL // FINE)
    if per.sum() <= large_cap:
        return [int(per.sum())]
    out, g = [], 0
    for c in per[per > 0]:
        if g and g + c > large_cap:
            out.append(g)
            g = 0
        g += int(c)
    return out + [g]


def predict_classes(pairs, small_cap, large_cap):
    """(small class slabs, large class slabs) of the pairs' rows"""
    sizes = [z for rows in pairs for z in predict_slabs(rows, large_cap)]
    assert max(sizes) <= large_cap
    small = sum(1 for z in sizes if z <= small_cap)
    return small, len(sizes) - small


def spread_rows(n, lo=0, hi=PANEL):
    """n distinct rows, evenly spread over [lo, hi)"""
    return lo + (np.arange(n, dtype=np.int64) * (hi - lo)) // n


def operands(pairs, values, negate=False, seed=5):
    """A: for pair i the columns 2i (its rows) and 2i + 1 (EXTRA of them, the first and the
    last row included); B: column i = {2i, 2i + 1}.  values `int`: integers 1..4 in A and 1..2
    in B; `half`: the same with A's values + 0.5 (f32-exact, not integral: the f64 slabs)."""
    rng = np.random.default_rng(seed)
    acols = []
    for rows in pairs:
        rows = np.asarray(rows, np.int64)
        assert len(rows) > EXTRA and len(np.unique(rows)) == len(rows) and 0 <= rows.min() and rows.max() < PANEL
        rows = np.sort(rows)
        sub = np.sort(np.concatenate([rows[[0, -1]], rng.choice(rows[1:-1], EXTRA - 2, replace=False)]))
        acols += [rows, sub]
    na = sum(len(c) for c in acols)
    av = rng.integers(1, 5, na).astype(np.float64) + (0.5 if values == "half" else 0.0)
    Ah = H.dcsc_from_cols(PANEL, len(acols), acols, -av if negate else av)
    bcols = [np.array([2 * i, 2 * i + 1]) for i in range(len(pairs))]
    Bh = H.dcsc_from_cols(len(acols), len(bcols), bcols, rng.integers(1, 3, 2 * len(pairs)).astype(np.float64))
    return Ah, Bh


def multiply(cbg, Ah, Bh, sr):
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    try:
        C = cbg.LocalHybridSpGEMM(A, B, sr)
        w = {k: int(v) for k, v in cbg.last_work_stats().items()}
        st = cbg.last_stats()
        Ch = C.to_host()
        C.free()
    finally:
        A.free()
        B.free()
    return Ch, w, st


def check_route(w, st, pairs, iacc, caps):
    """int_accumulate, the two bitmap classes and the slab count against the prediction"""
    small_cap, large_cap = (caps[2], caps[3]) if iacc else (caps[0], caps[1])
    small, large = predict_classes(pairs, small_cap, large_cap)
    print("iacc", iacc, "caps", small_cap, large_cap, "predicted", small, large, {k: v for k, v in w.items() if v})
    assert w["int_accumulate"] == int(iacc), w
    assert w["bitmap_small_kept"] + w["bitmap_small_mark"] == small, (w, small, large)
    assert w["bitmap_large_kept"] + w["bitmap_large_mark"] == large, (w, small, large)
    assert st["n_slabs"] == small + large and st["n_big"] == len(pairs), st
    assert w["slab_over_cap"] == 0, w


def test_caps_are_the_derived_ones(cbg):
    """the f64 caps are the documented ones; the IACC caps fill the same LDS at 6 B per
    nonzero: 2 blocks of 512 threads per CU (2 x 81920 B) and one block of 1024 (163840 B),
    with the fixed part of the layout (bv, bm, pref, st, tmp, wpre) at 57408 / 65632 B"""
    caps = cbg.local_slab_caps()
    assert caps[:2] == [F64_SMALL, F64_LARGE]
    for cap, fixed, lds in ((caps[2], 57408, 81920), (caps[3], 65632, 163840)):
        assert cap % 8 == 0 and fixed + 6 * cap <= lds < fixed + 6 * (cap + 8), caps
    assert caps[2] > F64_SMALL and caps[3] > F64_LARGE and caps[3] < 65536


# ---------------------------------------------------------------------------------------
# 1. class edges
# ---------------------------------------------------------------------------------------
def edge_sizes(caps):
    return sorted({F64_SMALL, F64_SMALL + 1, caps[2], caps[2] + 1, F64_LARGE, F64_LARGE + 1, caps[3], caps[3] + 1})


@functools.lru_cache(maxsize=None)
def _edge_case(n, values, negate, sr):
    pairs = (spread_rows(n),)
    Ah, Bh = operands(pairs, values, negate, seed=n)
    return pairs, Ah, Bh, oracle_local(Ah, Bh, sr)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("values", ["int", "half"])
def test_class_edges(cbg, values, sr, negate):
    """one pair of exactly N nonzeros on either side of every cap: integers run IACC with its
    caps, half-integers the f64 slabs with theirs (3056 / 3057 and 12032 / 12033 whatever the
    IACC caps are)"""
    caps = cbg.local_slab_caps()
    for n in edge_sizes(caps):
        pairs, Ah, Bh, ref = _edge_case(n, values, negate, sr)
        C, w, st = multiply(cbg, Ah, Bh, sr)
        assert len(C["ir"]) == n
        assert_tiles_bits_equal(C, ref)
        check_route(w, st, pairs, values == "int", caps)
        if values == "half":
            small, large = predict_classes(pairs, F64_SMALL, F64_LARGE)
            assert (n > F64_SMALL or (small, large) == (1, 0)) and (not F64_SMALL < n <= F64_LARGE or
                                                                    (small, large) == (0, 1)), n
            assert small + large == (1 if n <= F64_LARGE else 2), n


def test_class_edges_prediction_moves_with_the_caps(cbg):
    """the prediction itself, without a multiply: a pair one above a class's cap leaves it"""
    caps = cbg.local_slab_caps()
    for small_cap, large_cap in ((caps[0], caps[1]), (caps[2], caps[3])):
        got = [predict_classes((spread_rows(n),), small_cap, large_cap)
               for n in (small_cap, small_cap + 1, large_cap, large_cap + 1)]
        assert got[:3] == [(1, 0), (0, 1), (0, 1)] and sum(got[3]) == 2, got


# ---------------------------------------------------------------------------------------
# 2. rebuilding rows from 16 bits and the rank
# ---------------------------------------------------------------------------------------
Q = 1 << 16
SPECIAL = np.array([0, Q - 1, Q, 2 * Q - 1, 2 * Q, 3 * Q - 1, 3 * Q, 4 * Q - 1], np.int64)


def _fill(must, n, lo, hi, rng, allowed=None):
    """n distinct rows of [lo, hi): `must` and random others (of the ranges `allowed`, pairs
    of row bounds, when given)"""
    pool = np.arange(lo, hi) if allowed is None else np.concatenate([np.arange(a, b) for a, b in allowed])
    pool = np.setdiff1d(pool, must)
    return np.sort(np.concatenate([must, rng.choice(pool, n - len(must), replace=False)]))


def rebuild_pairs(case, cls, caps):
    """the rows of one pair (see test_rebuilt_rows); cls: the IACC class of the slab in question"""
    rng = np.random.default_rng(17)
    n = caps[2] - 500 if cls == "small" else caps[2] + 500
    if case == "quarters":      # lo = 0: the first and the last row of each 2^16 range above it
        return _fill(SPECIAL, n, 0, PANEL, rng)
    if case == "second_slab":
        # fine ranges 0..2 hold 20 fewer than the large IACC cap, so the first slab ends with
        # them and the second starts at lo = 3 * 8192: a multiple of 8192, not of 65536
        lo = 3 * FINE
        head = spread_rows(caps[3] - 20, 0, lo)
        sp = lo + SPECIAL[SPECIAL < PANEL - lo]
        tail = _fill(np.concatenate([sp, [PANEL - 1]]), n, lo, PANEL, rng)
        assert PANEL - lo > Q
        return np.concatenate([head, tail])
    if case == "empty_middle":  # no row in the second and third 2^16 range: t1 = t2 = t3
        return _fill(np.array([0, Q - 1, 3 * Q, 4 * Q - 1]), n, 0, PANEL, rng, [(0, Q), (3 * Q, 4 * Q)])
    if case == "empty_top":     # the slab ends inside the second range: t2 = t3 = nout
        return _fill(np.array([0, Q - 1, Q, Q + FINE - 1]), n, 0, Q + FINE, rng)
    raise KeyError(case)


@pytest.mark.parametrize("cls", ["small", "large"])
@pytest.mark.parametrize("case", ["quarters", "second_slab", "empty_middle", "empty_top"])
def test_rebuilt_rows(cbg, case, cls):
    """rows at lo + {0, 65535, 65536, 131071, 131072, 196607, 196608, 262143}; the same in the
    second slab of a two-slab pair whose lo is a multiple of 8192 but not of 65536 and which
    spans more than 2^16 rows; slabs with no row in one or two of the four 2^16 ranges (equal
    thresholds, thresholds equal to the slab's nonzeros) -- in both classes, both semirings"""
    caps = cbg.local_slab_caps()
    pairs = (rebuild_pairs(case, cls, caps),)
    sizes = predict_slabs(pairs[0], caps[3])
    assert len(sizes) == (2 if case == "second_slab" else 1), sizes
    assert (sizes[-1] <= caps[2]) == (cls == "small"), sizes
    Ah, Bh = operands(pairs, "int")
    for sr in ("plus", "minplus"):
        C, w, st = multiply(cbg, Ah, Bh, sr)
        np.testing.assert_array_equal(C["ir"], np.sort(pairs[0]))
        assert_tiles_bits_equal(C, oracle_local(Ah, Bh, sr))
        check_route(w, st, pairs, True, caps)


# ---------------------------------------------------------------------------------------
# 3. cuts at the new large cap
# ---------------------------------------------------------------------------------------
_MARKING_CODE = r"""
import json, sys
import numpy as np
from conftest import load_cbg
import test_gpu_slab_lds as T
cbg = load_cbg()
caps = cbg.local_slab_caps()
pairs = (T.spread_rows(caps[3] + 1),)
Ah, Bh = T.operands(pairs, "int")
C, w, st = T.multiply(cbg, Ah, Bh, sys.argv[1])
np.savez(sys.argv[2], **{k: C[k] for k in ("cp", "jc", "ir", "val")})
print(json.dumps(w))
"""


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_cuts_at_the_large_cap(cbg, monkeypatch, tmp_path, sr):
    """a pair of one more nonzero than the large IACC cap, so two slabs with cuts: with the
    symbolic's cuts, with the numeric's searches (CBG_CUTS_CAP=0), with the map hops
    (CBG_STAGE_RUNS=0) and with the marking pass (CBG_BITMAP_BUDGET_GB=0, read once per
    process: a child process) C is the same, the oracle's"""
    caps = cbg.local_slab_caps()
    pairs = (spread_rows(caps[3] + 1),)
    Ah, Bh = operands(pairs, "int")
    ref = oracle_local(Ah, Bh, sr)
    for env in (None, "CBG_CUTS_CAP", "CBG_STAGE_RUNS"):
        if env:
            monkeypatch.setenv(env, "0")
        C, w, st = multiply(cbg, Ah, Bh, sr)
        if env:
            monkeypatch.delenv(env)
        assert_tiles_bits_equal(C, ref)
        check_route(w, st, pairs, True, caps)
        assert st["n_slabs"] == 2 and w["bitmap_small_kept"] + w["bitmap_large_kept"] == 2, (env, w)
        assert w["staged_multiplies"] == (0 if env == "CBG_STAGE_RUNS" else 1), (env, w)
    out = str(tmp_path / "c.npz")
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path.insert(0, %r)\n" % tests + _MARKING_CODE, sr, out],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, CBG_BITMAP_BUDGET_GB="0"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    w = json.loads(r.stdout.strip().splitlines()[-1])
    assert w["bitmap_small_mark"] + w["bitmap_large_mark"] == 2 and w["int_accumulate"] == 1, w
    assert w["bitmap_small_kept"] + w["bitmap_large_kept"] == 0, w
    z = np.load(out)
    assert_tiles_bits_equal(dict(m=ref["m"], n=ref["n"], cp=z["cp"], jc=z["jc"], ir=z["ir"], val=z["val"]), ref)


# ---------------------------------------------------------------------------------------
# 4. the verdict across the pieces of one phased multiply
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("half_piece", [1, 0])
@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_verdict_across_pieces(cbg, sr, half_piece):
    """a forced two-phase MemEfficientSpGEMM, one pair per piece, each of more nonzeros than an
    f64 slab holds and no more than a large IACC slab: the integral piece runs IACC with one
    slab, the piece whose B carries one 0.5 runs the f64 slabs with two -- in either order --
    the check on the plan counts nothing, and the second piece takes A's maps and verdicts
    from the call's cache"""
    caps = cbg.local_slab_caps()
    assert caps[3] > F64_LARGE + 1
    pairs = (spread_rows((F64_LARGE + 1 + caps[3]) // 2), spread_rows(caps[3]))
    Ah, Bh = operands(pairs, "int")
    Bh = dict(Bh, val=Bh["val"].copy())
    Bh["val"][2 * half_piece] = 0.5
    refs = [oracle_local(Ah, Bp, sr) for Bp in H.aprep_pieces(Bh, 2)]
    grid = _grid(cbg)
    A, B = _mat(cbg, grid, Ah), _mat(cbg, grid, Bh)
    try:
        got = _phased(cbg, A, B, 2, sr)
    finally:
        A.tile.free()
        B.tile.free()
        grid.destroy()
    assert [(ph, off) for ph, off, _, _ in got] == [(0, 0), (1, 1)]
    for p, (_, _, C, w) in enumerate(got):
        print(p, {k: v for k, v in w.items() if v})
        assert_tiles_bits_equal(C, refs[p])
        iacc = p != half_piece
        assert w["int_accumulate"] == int(iacc), (p, w)
        assert sum(w[k] for k in BITMAP) == (1 if iacc else 2), (p, w)
        assert w["bitmap_small_mark"] + w["bitmap_large_mark"] == 0, (p, w)
        assert w["slab_over_cap"] == 0, (p, w)
        assert (w["amap_reused"], w["pmap_reused"], w["avals_reused"]) == ((0, 0, 0) if p == 0 else (1, 1, 1)), (p, w)


# ---------------------------------------------------------------------------------------
# 5. R-MAT against the golden digests
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [None, "64"])
@pytest.mark.parametrize("scale", [12, 14])
def test_rmat_digests(cbg, monkeypatch, scale, big):
    """scale 12 and 14 (one row panel, multi-slab hub columns), default cut and
    CBG_BIG_FLOPS=64: the integer product (IACC) against the golden digests by bits; with
    U[-1, 1) values (the f64 slabs) the golden structure, and at scale 12 every value against
    the oracle within 1e-12 (|A||B|)ij"""
    if big:
        monkeypatch.setenv("CBG_BIG_FLOPS", big)
    g = golden()["rmat"][f"s{scale}_ef16"]
    for sr, key in (("plus", "C_local_plus"), ("minplus", "C_local_minplus")):
        A = cbg.rmat_tile(scale, 16)
        C = cbg.LocalHybridSpGEMM(A, A, sr)
        w = {k: int(v) for k, v in cbg.last_work_stats().items()}
        assert_digest_eq(C.digest(), g[key])
        assert w["int_accumulate"] == 1 and sum(w[k] for k in BITMAP) > 0 and w["slab_over_cap"] == 0, w
        C.free()
        A.set_random_values()
        C = cbg.LocalHybridSpGEMM(A, A, sr)
        w = {k: int(v) for k, v in cbg.last_work_stats().items()}
        assert_digest_eq(C.digest(), g[key], values=False)
        assert w["int_accumulate"] == 0 and sum(w[k] for k in BITMAP) > 0 and w["slab_over_cap"] == 0, w
        if scale == 12:
            Ah, Ch = A.to_host(), C.to_host()
            ref = oracle_local(Ah, dict(Ah), sr)
            if sr == "plus":
                assert_tiles_equal(Ch, ref, rtol=1e-12, bound=oracle_local(abs_tile(Ah), abs_tile(Ah))["val"])
            else:
                assert_tiles_equal(Ch, ref)
        C.free()
        A.free()
