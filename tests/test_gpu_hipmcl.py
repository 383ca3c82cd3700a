"""The HipMCL iteration on device (csrc/cbg_mcl.hip, the loop in csrc/cbg_grid_algos.cpp)
against the NumPy restatement (tests/hipmcl_ref.py).  Where the inputs' sums are exact
(dyadic values) results are compared by bits; on inexact values the column sums, moments
and the inflation are compared by bits with the order-exact restatement (tests/colsum_ref.py,
whose own checks are in tests/test_colsum_cpu.py).

Tolerances (measured, see DESIGN.md "HipMCL iteration"):
  POW_ULP   device pow against numpy.power over the 109419 values of test_apply_pow: the
            largest distance measured is 1 ulp; the bound is twice that.
  CHAOS_RTOL  chaos per iteration, |device - restatement| / max(restatement, EPS): below
            EPS = 1e-4 (the loop's own threshold) a chaos only says "converged", and it is
            a difference of two numbers near 1, so its error does not shrink with it.
            Measured: restatement against the reference's own Chaos dump 4.9e-16 (on the
            host, tests/test_hipmcl_cpu.py); device against restatement over the four
            end-to-end cases 9.56e-14 (the device multiply's sum order differs from the
            oracle's and changes from run to run).  The bound is ten times the larger.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import colsum_ref as cr
import hipmcl_ref as hr
import mcl_ref
from helpers import assert_tiles_bits_equal
from test_multiprocess import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
POW_ULP = 2
CHAOS_RTOL = 9.56e-13


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


@pytest.fixture
def grid(cbg):
    g = _self_grid(cbg)
    yield g
    g.destroy()


def _mat(cbg, g, d):
    return cbg.SpParMat(cbg.Tile.from_dict(d), g, d["m"], d["n"])


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _big():
    return mcl_ref.big_case()


@functools.lru_cache(maxsize=None)
def _big_positive():
    """big_case without its negative and zero entries"""
    t = _big()
    keep = t["val"] > 0
    return hr.from_coo(t["m"], t["n"], t["ir"][keep], hr.cols_of(t)[keep], t["val"][keep])


@functools.lru_cache(maxsize=None)
def _class_tile():
    """columns of length b - 1, b, b + 1 of the column-moment classes' bounds (16, 4096)"""
    rng = np.random.default_rng(11)
    cols = [mcl_ref.dyadic(rng, ln) for ln in (15, 16, 17, 4095, 4096, 4097)]
    return mcl_ref.build_tile(rng, 8192, 12, cols)


# ---------------------------------------------------------------------------
# column reductions
# ---------------------------------------------------------------------------
def test_moment_bounds_are_the_tested_ones(cbg):
    assert cbg.mcl_moment_bounds() == [16, 4096]
    lens = set(np.diff(_class_tile()["cp"]).tolist())
    assert {b + d for b in cbg.mcl_moment_bounds() for d in (-1, 0, 1)} <= lens
    assert max(np.diff(_big()["cp"])) == 30000


@pytest.mark.parametrize("case", ["small", "big", "classes"])
def test_reduce_cols_bit_equal(cbg, grid, case):
    t = {"small": lambda: mcl_ref.small_case(1), "big": _big, "classes": _class_tile}[case]()
    A = _mat(cbg, grid, t)
    empty = np.setdiff1d(np.arange(t["n"]), t["jc"])
    assert len(empty) > 0
    for what, ident in (("sum", 0.0), ("sum", -7.5), ("max", 0.0), ("max", -1e300), ("max", hr.DBL_MIN),
                        ("sumsq", 0.0), ("count", 0.0)):
        got = A.Reduce(cbg.Column, what, ident)
        want = hr.reduce_cols(t, what, ident)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{what} {ident}")
        assert np.all(got[empty] == ident)
    if case != "classes":  # max with identity 0 on an all-negative column
        neg = [j for p, j in enumerate(t["jc"]) if np.all(t["val"][t["cp"][p]:t["cp"][p + 1]] < 0)]
        assert neg and np.all(A.Reduce(cbg.Column, "max", 0.0)[neg] == 0.0)
        assert np.all(A.Reduce(cbg.Column, "max", -1e300)[neg] < 0.0)
    again = A.Reduce(cbg.Column, "sum", 0.0)  # the same bits in every run
    np.testing.assert_array_equal(_bits(again), _bits(hr.reduce_cols(t, "sum", 0.0)))


def test_reduce_negative_zero_column_and_unknown_ops(cbg, grid):
    """documented in cbg.h: the sums start from +0.0, so a column of -0.0 only sums to +0.0
    (a host sum gives -0.0); its maximum is -0.0 and its count 2.  An unknown op is an
    INVALIDPARAMS error of the mirror, not a ctypes one."""
    t = hr.from_coo(8, 3, [1, 5, 2], [0, 0, 2], [-0.0, -0.0, 0.5])
    A = _mat(cbg, grid, t)
    for what in ("sum", "sumsq"):
        got = A.Reduce(cbg.Column, what, 0.0)
        np.testing.assert_array_equal(_bits(got[:1]), _bits([0.0]))
    np.testing.assert_array_equal(_bits(A.Reduce(cbg.Column, "max", -1.0)), _bits([-0.0, -1.0, 0.5]))
    np.testing.assert_array_equal(A.Reduce(cbg.Column, cbg.RED_COUNT, 0.0), [2.0, 0.0, 1.0])
    for call in (lambda: A.Reduce(cbg.Column, "median"), lambda: A.Reduce(cbg.Column, 7), lambda: A.Reduce(cbg.Column, None),
                 lambda: A.Apply("exp", 2.0), lambda: A.Apply(3, 2.0)):
        with pytest.raises(cbg.CbgError) as e:
            call()
        assert e.value.code == cbg.INVALIDPARAMS


# ---------------------------------------------------------------------------
# MakeColStochastic, Apply
# ---------------------------------------------------------------------------
def test_make_col_stochastic_bit_equal(cbg, grid):
    t = _big_positive()
    A = _mat(cbg, grid, t)
    A.MakeColStochastic()
    assert_tiles_bits_equal(A.tile.to_host(), hr.make_col_stochastic(t))


def test_make_col_stochastic_zero_sum_column(cbg, grid):
    """a column whose only entries are 0.0: inv = DBL_MAX, DBL_MAX * 0 = 0"""
    t = hr.from_coo(8, 4, [0, 3, 1, 2, 5], [1, 1, 2, 2, 2], [0.0, 0.0, 0.25, 0.5, 0.25])
    A = _mat(cbg, grid, t)
    A.MakeColStochastic()
    got = A.tile.to_host()
    assert_tiles_bits_equal(got, hr.make_col_stochastic(t))
    np.testing.assert_array_equal(_bits(got["val"]), _bits([0.0, 0.0, 0.25, 0.5, 0.25]))


def _ulp_distance(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)  # positive doubles: the bit patterns are ordered
    return np.abs(ia - ib)


def test_apply_pow(cbg, grid):
    t = _big()
    A = _mat(cbg, grid, t)
    A.Apply("pow", 2.0)
    assert_tiles_bits_equal(A.tile.to_host(), dict(t, val=t["val"] * t["val"]))
    p = hr.make_col_stochastic(_big_positive())  # values in (0, 1], not dyadic
    B = _mat(cbg, grid, p)
    B.Apply("pow", 1.7)
    got = B.tile.to_host()["val"]
    want = np.power(p["val"], 1.7)
    d = _ulp_distance(got, want)
    print("pow(v, 1.7) against numpy.power: largest distance %d ulp over %d values" % (int(d.max()), len(d)))
    assert d.max() <= POW_ULP


# ---------------------------------------------------------------------------
# the fused inflation against the four-call composition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("power", [2.0, 1.7])
def test_inflate_fused_equals_composed(cbg, grid, power):
    t = hr.make_col_stochastic(_big_positive())
    t = dict(t, val=t["val"] * 0.75)  # not normalised any more: the first pass has work to do
    F, C = _mat(cbg, grid, t), _mat(cbg, grid, t)
    cf = F.Inflate(power)
    C.MakeColStochastic()
    cc = C.Chaos()
    C.Apply("pow", power)
    C.MakeColStochastic()
    assert np.float64(cf).view(np.uint64) == np.float64(cc).view(np.uint64), (cf, cc)
    assert_tiles_bits_equal(F.tile.to_host(), C.tile.to_host())
    st = cbg.inflate_stats()
    assert st["nnz"] == len(t["ir"]) and all(ms > 0 for ms in st["ms"])
    # the restatement sums in another order: a sum of n <= 30000 positive terms is off by at
    # most n eps = 7e-12 relative, and three of them meet in a value; 1e-9 is a sanity bound
    # far above that (the bits are pinned by the composition above)
    want, wc = hr.inflate(t, power)
    assert abs(cf - wc) <= 1e-9 * max(wc, 1.0)
    np.testing.assert_allclose(F.tile.to_host()["val"], want["val"], rtol=1e-9)


def test_chaos_exact_on_dyadic(cbg, grid):
    t = _big()
    assert _mat(cbg, grid, t).Chaos() == hr.chaos(t)


# ---------------------------------------------------------------------------
# inexact values: the bits of the order-exact restatement (tests/colsum_ref.py)
# ---------------------------------------------------------------------------
def _assert_bits_or_nan(got, want, msg=""):
    """equal bits, and a NaN exactly where the restatement has one"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(msg))
    ok = ~np.isnan(want)
    bad = np.flatnonzero(_bits(got[ok]) != _bits(want[ok]))
    assert len(bad) == 0, (msg, "first of %d:" % len(bad), int(np.flatnonzero(ok)[bad[0]]), got[ok][bad[0]].hex(),
                           want[ok][bad[0]].hex())


def _assert_cols_bits(t, got, want, msg):
    """dense per-column results by bits; reports the first failing (length, got, want)"""
    bad = np.flatnonzero(_bits(got) != _bits(want))
    lens = cr.column_lengths(t)
    assert len(bad) == 0, (msg, "%d columns differ; first: length %d, got %s, want %s" % (
        len(bad), lens[bad[0]], float(got[bad[0]]).hex(), float(want[bad[0]]).hex()))


def _assert_vals_bits(t, got, want, msg):
    assert np.array_equal(got["cp"], want["cp"]) and np.array_equal(got["ir"], want["ir"])
    bad = np.flatnonzero(_bits(got["val"]) != _bits(want["val"]))
    lens = np.repeat(np.diff(t["cp"]), np.diff(t["cp"]))
    assert len(bad) == 0, (msg, "%d values differ; first: column length %d, got %s, want %s" % (
        len(bad), lens[bad[0]] if len(bad) else 0, float(got["val"][bad[0]]).hex(), float(want["val"][bad[0]]).hex()))


REDUCTIONS = (("sum", 0.0), ("sum", -7.5), ("sumsq", 0.0), ("sumsq", 3.0), ("max", 0.0), ("max", -1e300),
              ("count", 0.0), ("count", 9.0))


@pytest.mark.parametrize("pattern", cr.PATTERNS)
def test_reduce_cols_ordered_bits(cbg, grid, pattern):
    t = cr.inexact_case(pattern)
    A = _mat(cbg, grid, t)
    for what, ident in REDUCTIONS:
        got = A.Reduce(cbg.Column, what, ident)
        _assert_cols_bits(t, got, cr.reduce_cols_ordered(t, what, ident), (pattern, what, ident))
    again = A.Reduce(cbg.Column, "sum", 0.0)  # the same bits in every run
    np.testing.assert_array_equal(_bits(again), _bits(A.Reduce(cbg.Column, "sum", 0.0)))
    _assert_cols_bits(t, again, cr.reduce_cols_ordered(t, "sum"), (pattern, "again"))


@pytest.mark.parametrize("pattern", ["uniform", "wide"])
def test_make_col_stochastic_ordered_bits(cbg, grid, pattern):
    t = cr.inexact_case(pattern)
    A = _mat(cbg, grid, t)
    A.MakeColStochastic()
    _assert_vals_bits(t, A.tile.to_host(), cr.make_col_stochastic_ordered(t), pattern)


@pytest.mark.parametrize("pattern", cr.PATTERNS)
def test_chaos_ordered_bits(cbg, grid, pattern):
    t = cr.inexact_case(pattern)
    got, want = _mat(cbg, grid, t).Chaos(), cr.chaos_ordered(t)
    assert _bits([got])[0] == _bits([want])[0], (pattern, float(got).hex(), float(want).hex())
    if pattern == "uniform":  # a stochastic matrix's chaos: the figure the loop watches
        s = cr.make_col_stochastic_ordered(t)
        got, want = _mat(cbg, grid, s).Chaos(), cr.chaos_ordered(s)
        assert want > 0.0 and _bits([got])[0] == _bits([want])[0], (float(got).hex(), float(want).hex())


@pytest.mark.parametrize("pattern", ["uniform", "wide"])
def test_inflate_square_ordered_bits(cbg, grid, pattern):
    t = cr.inexact_case(pattern)
    A = _mat(cbg, grid, t)
    c = A.Inflate(2.0)
    want, wc = cr.inflate_ordered(t, 2.0)
    assert _bits([c])[0] == _bits([wc])[0], (pattern, float(c).hex(), float(wc).hex())
    _assert_vals_bits(t, A.tile.to_host(), want, pattern)


def test_inflate_power_ordered_bits(cbg, grid):
    """the device's pow cannot be restated by bits, so it is taken from the device: v = val * inv
    is computed here, raised to 1.7 by Apply, and the sums and the scaling are finished here"""
    t = cr.inexact_case("uniform")

    def device_pow(v):
        P = _mat(cbg, grid, dict(t, val=v))
        P.Apply("pow", 1.7)
        return P.tile.to_host()["val"]

    want, wc = cr.inflate_ordered(t, 1.7, pow_fn=device_pow)
    A = _mat(cbg, grid, t)
    c = A.Inflate(1.7)
    assert _bits([c])[0] == _bits([wc])[0], (float(c).hex(), float(wc).hex())
    _assert_vals_bits(t, A.tile.to_host(), want, "1.7")


def test_special_value_columns(cbg, grid):
    """+inf, a sum that cancels to exactly 0, subnormal sums, DBL_MIN and -0.0 entries in each
    length class, under IEEE rules"""
    t, cases = cr.special_case()
    A = _mat(cbg, grid, t)
    for what, ident in REDUCTIONS:
        _assert_bits_or_nan(A.Reduce(cbg.Column, what, ident), cr.reduce_cols_ordered(t, what, ident), (what, ident))
    got, want = A.Chaos(), cr.chaos_ordered(t)
    assert _bits([got])[0] == _bits([want])[0], (got, want)
    for strict in (1, 0):  # thr 0: -0.0 is kept only when not strict, its sum +0.0 either way
        cnt, tot = A.tile.col_stats(0.0, strict)
        wc, ws = cr.col_stats_ordered(t, np.zeros(t["n"]), strict)
        np.testing.assert_array_equal(cnt, wc)
        _assert_bits_or_nan(tot, ws, ("col_stats", strict))
    A.MakeColStochastic()
    g, w = A.tile.to_host(), cr.make_col_stochastic_ordered(t)
    _assert_bits_or_nan(g["val"], w["val"], "MakeColStochastic")
    # the restatement holds what the cases are about
    by = {c: w["val"][t["cp"][p]:t["cp"][p + 1]] for p, c in enumerate(cases)}
    src = {c: t["val"][t["cp"][p]:t["cp"][p + 1]] for p, c in enumerate(cases)}
    sums = cr.reduce_cols_ordered(t, "sum")[t["jc"]]
    for p, (kind, ln) in enumerate(cases):
        v = by[(kind, ln)]
        if kind == "inf":
            assert sums[p] == np.inf and np.isnan(v).sum() == 1 and np.all(v[~np.isnan(v)] == 0.0)
        elif kind == "cancel":
            assert _bits([sums[p]])[0] == 0 and np.all(np.abs(v[3:]) == hr.DBL_MAX) and v[0] == np.inf
        elif kind == "subnormal":
            assert 0.0 < sums[p] < hr.DBL_MIN and np.all(v == np.inf)
        elif kind == "dbl_min":
            assert sums[p] == ln * hr.DBL_MIN and np.all(np.abs(v * ln - 1.0) < 1e-14)
        else:
            assert _bits([sums[p]])[0] == 0 and np.all(_bits(v) == _bits([-0.0])[0]) and np.all(src[(kind, ln)] == 0)


@pytest.mark.parametrize("nnz", [1, 2, 3, 4, 517])
def test_apply_pow_unaligned_head(cbg, nnz):
    """k_apply_pow's head path: a val that starts 8 bytes off a 16-byte boundary, as a borrowed
    view of a tile's entries from its second one on"""
    import ctypes
    rng = np.random.default_rng(nnz)
    v = rng.uniform(0.5, 2.0, nnz + 1)
    base = cbg.Tile.from_dict(hr.from_coo(nnz + 1, 1, np.arange(nnz + 1), np.zeros(nnz + 1), v))
    assert base.c.val % 16 == 0
    view = cbg.CTile(base.c.m, 1, nnz, 1, base.c.cp, base.c.jc, base.c.ir + 4, base.c.val + 8, 1, 0)
    assert cbg.lib().cbg_tile_apply(ctypes.byref(view), cbg.APPLY_POW, 2.0) == 0
    got = base.to_host()["val"]
    np.testing.assert_array_equal(_bits(got), _bits(np.concatenate([v[:1], v[1:] * v[1:]])))


# ---------------------------------------------------------------------------
# loops
# ---------------------------------------------------------------------------
def _loops_long_case():
    """300 x 300 with columns of more than one 64-lane round around their diagonal: 150 stores it
    at position 65 of 130, 200 at position 64 of 130, 100 (65 entries) lacks it and gains it at
    position 64 with one entry behind; short columns beside them"""
    cols = {150: list(range(85, 215)), 200: list(range(136, 266)), 100: list(range(36, 100)) + [200],
            3: [3], 7: [1, 299], 299: [0, 150]}
    row = [r for j in sorted(cols) for r in cols[j]]
    col = [j for j in sorted(cols) for _ in cols[j]]
    return hr.from_coo(300, 300, row, col, (np.arange(len(row)) % 97 + 1) / 128.0)


@pytest.mark.parametrize("n", [1, 4, 5, 2048, 2049, "long"])
def test_loops_slot_counts(cbg, grid, n):
    """the same on n dense columns: one slot that is first and last at once and holds only its
    loop (1: RemoveLoops gives the empty tile, AddLoops fills a tile that stores nothing), a wave
    per column in blocks of four (4, 5), the column scan's one tile and its second level (2048,
    2049), where columns 0 and n - 1 store nothing, so the first and the last slot gain an entry
    under AddLoops and stay empty under RemoveLoops; long: the dropped, replaced or inserted entry
    at position 64 and 65 of a column, entries behind it (_loops_long_case)"""
    if n == "long":
        t = _loops_long_case()
    elif n == 1:
        t = hr.from_coo(1, 1, [0], [0], [0.5])
    elif n <= 16:
        t = hr.from_coo(n, n, [1, 2, 2, 1], [1, 1, 2, n - 2], [0.5, 0.25, 0.125, 0.75])
    else:
        t = hr.loops_case(seed=n, n=n)
    n = t["n"]
    A = _mat(cbg, grid, t)
    want, removed = hr.remove_loops(t)
    assert A.RemoveLoops() == removed > 0
    assert A.tile.digest()["unsorted"] == 0
    assert_tiles_bits_equal(A.tile.to_host(), want)
    if n == 1:
        assert removed == 1 and A.tile.nnz == 0 and A.tile.nzc == 0
    lv = (np.arange(n) + 1) / 64.0
    for src in (t, want):
        for replace in (True, False):
            B = _mat(cbg, grid, src)
            B.AddLoops(lv, replace)
            assert B.tile.digest()["unsorted"] == 0 and B.tile.nzc == n
            assert_tiles_bits_equal(B.tile.to_host(), hr.add_loops(src, lv, replace))


def test_loops_against_restatement(cbg, grid):
    t = hr.loops_case()
    n = t["n"]
    col, row = hr.cols_of(t), t["ir"].astype(np.int64)
    stored = set(col[col == row].tolist())
    first = {int(j): int(t["ir"][t["cp"][p]]) for p, j in enumerate(t["jc"])}
    last = {int(j): int(t["ir"][t["cp"][p + 1] - 1]) for p, j in enumerate(t["jc"])}
    lens = dict(zip(t["jc"].tolist(), np.diff(t["cp"]).tolist()))
    empty = set(range(n)) - set(lens)
    # the input holds what the test is about
    assert stored and set(lens) - stored and empty
    assert any(first[j] == j and lens[j] > 1 for j in stored) and any(last[j] == j and lens[j] > 1 for j in stored)
    assert any(first[j] < j < last[j] for j in stored) and any(lens[j] == 1 for j in stored)
    A = _mat(cbg, grid, t)
    want, removed = hr.remove_loops(t)
    assert A.RemoveLoops() == removed == len(stored)
    assert A.tile.digest()["unsorted"] == 0
    assert_tiles_bits_equal(A.tile.to_host(), want)
    assert A.RemoveLoops() == 0
    lv = (np.arange(n) + 1) / 64.0
    for src in (t, want):  # with stored loops, and with none (emptied and empty columns gain one)
        for replace in (False, True):
            B = _mat(cbg, grid, src)
            B.AddLoops(lv, replace)
            assert B.tile.digest()["unsorted"] == 0
            assert_tiles_bits_equal(B.tile.to_host(), hr.add_loops(src, lv, replace))
    keep = hr.add_loops(t, lv, False)["val"]
    repl = hr.add_loops(t, lv, True)["val"]
    assert np.sum(keep != repl) == len(stored)
    B = _mat(cbg, grid, want)
    B.AddLoops(0.5)  # one value for every vertex
    assert_tiles_bits_equal(B.tile.to_host(), hr.add_loops(want, 0.5))
    C = _mat(cbg, grid, t)
    C.AdjustLoops()
    got = C.tile.to_host()
    assert C.tile.digest()["unsorted"] == 0
    assert_tiles_bits_equal(got, hr.adjust_loops(t))
    d = got["val"][hr.cols_of(got) == got["ir"]]
    assert len(d) == n and np.sum(d == hr.DBL_MIN) >= len(empty)  # the quirk: an empty column's loop
    C.MakeColStochastic()
    s = C.tile.to_host()
    assert np.all(s["val"][np.isin(hr.cols_of(s), list(empty))] == 1.0)


def test_loops_refuse_rectangular(cbg, grid):
    t = hr.from_coo(6, 5, [0, 1], [0, 1], [0.5, 0.5])
    A = _mat(cbg, grid, t)
    for call in (A.RemoveLoops, A.AdjustLoops, lambda: A.AddLoops(1.0)):
        with pytest.raises(cbg.CbgError) as e:
            call()
        assert e.value.code == cbg.DIMMISMATCH


# ---------------------------------------------------------------------------
# connected components
# ---------------------------------------------------------------------------
def _cc_cases():
    rng = np.random.default_rng(5)
    n = 4096
    perm = rng.permutation(n)
    yield "path_shuffled", n, perm[:-1], perm[1:]
    yield "star", 1000, np.full(999, 617), np.delete(np.arange(1000), 617)
    yield "isolated", 1000, np.zeros(0, np.int64), np.zeros(0, np.int64)
    a = rng.permutation(600)
    yield "directed_only", 600, a[:-1:2], a[1::2]  # pairs (i, j) stored once, never (j, i)
    r1, c1 = rng.integers(0, 1500, 6000), rng.integers(0, 1500, 6000)
    r2, c2 = rng.integers(1500, 3000, 6000), rng.integers(1500, 3000, 6000)
    yield "two_joined", 3000, np.concatenate([r1, r2, [2999]]), np.concatenate([c1, c2, [0]])
    yield "two_apart", 3000, np.concatenate([r1, r2]), np.concatenate([c1, c2])
    yield "empty", 0, np.zeros(0, np.int64), np.zeros(0, np.int64)


@pytest.mark.parametrize("name", [c[0] for c in _cc_cases()])
def test_connected_components_exact(cbg, grid, name):
    _, n, rows, cols = next(c for c in _cc_cases() if c[0] == name)
    key = np.unique(np.asarray(rows, np.int64) * max(n, 1) + np.asarray(cols, np.int64))
    rows, cols = (key // max(n, 1), key % max(n, 1)) if n else (key, key)
    t = hr.from_coo(n, n, rows, cols, np.ones(len(rows)))
    want = hr.components(n, rows, cols)
    got = cbg.Interpret(_mat(cbg, grid, t))
    np.testing.assert_array_equal(got, want)
    if name == "path_shuffled":
        assert got.max() == 0
    if name == "isolated":
        np.testing.assert_array_equal(got, np.arange(n))
    if name == "two_joined":
        apart = next(c for c in _cc_cases() if c[0] == "two_apart")
        assert want.max() + 1 < hr.components(n, apart[2], apart[3]).max() + 1


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restated(case, ps):
    t = hr.CASES[case]()
    return t, hr.hipmcl(t, *ps)


@pytest.mark.parametrize("ps", hr.PARAM_SETS, ids=["i2_select", "i1.7_threshold"])
@pytest.mark.parametrize("case", sorted(hr.CASES))
def test_hipmcl_end_to_end(cbg, grid, case, ps):
    t, (wlab, wit, wchaos, _) = _restated(case, ps)
    infl, h, S, R, q = ps
    A = _mat(cbg, grid, t)
    seen = []
    labels, its, F = cbg.HipMCL(A, inflation=infl, prunelimit=h, select=S, recover_num=R, recover_pct=q,
                                on_iteration=lambda *a: seen.append(a), keep_final=True)
    assert_tiles_bits_equal(A.tile.to_host(), t)  # the input is left as it was
    assert its == wit == len(seen) and [a[0] for a in seen] == list(range(1, its + 1))
    np.testing.assert_array_equal(labels, wlab)  # canonical labels: equal partitions
    rel = [abs(a[1] - w) / max(w, hr.EPS) for a, w in zip(seen, wchaos)]
    print("chaos against the restatement, %s %s: largest relative difference %.3g" % (case, ps, max(rel)))
    assert max(rel) <= CHAOS_RTOL, rel
    # the reference's own run of the case
    z = hr.load_golden(case)
    k = hr.PARAM_SETS.index(ps)
    assert tuple(z["params"][k]) == ps and its == int(z[f"iterations{k}"])
    np.testing.assert_array_equal(labels, z[f"labels{k}"])
    assert all(hr.printed_agrees(a[1], p) for a, p in zip(seen, z[f"printed{k}"])), (seen, z[f"printed{k}"])
    # invariants of the final matrix
    f = F.tile.to_host()
    assert F.tile.digest()["unsorted"] == 0 and len(f["jc"]) == t["n"]
    lens = np.diff(f["cp"])
    sums = np.array([np.sum(f["val"][f["cp"][p]:f["cp"][p + 1]]) for p in range(len(lens))])
    assert np.all(np.abs(sums - 1.0) <= 4 * np.finfo(np.float64).eps * lens)
    st = cbg.hipmcl_stats()
    assert seen[-1][1] <= hr.EPS and st["chaos"] == seen[-1][1] and st["iterations"] == its
    assert st["final_nnz"] == len(f["ir"]) == seen[-1][2]
    np.testing.assert_array_equal(labels, hr.interpret(f))
    np.testing.assert_array_equal(cbg.Interpret(F), labels)


def test_hipmcl_iteration_cap_and_callback(cbg, grid):
    t = hr.planted()
    A = _mat(cbg, grid, t)
    seen = []
    labels, its = cbg.HipMCL(A, select=8, recover_num=10, max_iterations=1, on_iteration=lambda *a: seen.append(a))
    assert its == 1 and len(seen) == 1 and cbg.hipmcl_stats()["chaos"] > hr.EPS
    want = hr.hipmcl(t, 2.0, 1e-4, 8, 10, 0.9, max_iterations=1)
    np.testing.assert_array_equal(labels, want[0])
    labels3, its3 = cbg.HipMCL(A, select=8, recover_num=10, max_iterations=3)
    assert its3 == 3
    with pytest.raises(ZeroDivisionError):  # a callback's exception surfaces after the loop
        cbg.HipMCL(A, select=8, recover_num=10, max_iterations=2, on_iteration=lambda *a: 1 / 0)
    for bad in (dict(inflation=float("nan")), dict(inflation=-2.0), dict(max_iterations=-1), dict(select=-1)):
        with pytest.raises(cbg.CbgError) as e:
            cbg.HipMCL(A, **bad)
        assert e.value.code == cbg.INVALIDPARAMS


def test_hipmcl_preprune_rule(cbg, grid):
    """average degree > max(S, R) prunes before the first iteration (MCL.cpp:531-538)"""
    t = hr.planted()
    A = _mat(cbg, grid, t)
    for pre in (None, True, False):
        labels, its = cbg.HipMCL(A, select=4, recover_num=5, preprune=pre)
        want = hr.hipmcl(t, 2.0, 1e-4, 4, 5, 0.9, preprune=pre)
        assert its == want[1], pre
        np.testing.assert_array_equal(labels, want[0])
    assert len(hr.adjust_loops(t)["ir"]) // t["n"] > 5  # the rule fires for None


def _fnv1a_labels(labels):
    h = 0xcbf29ce484222325
    for b in np.asarray(labels, "<i8").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_hipmcl_check_driver(cbg, grid, tmp_path):
    """tools/hipmcl_check on the C++ mirror header against the Python mirror: R-MAT scale 10,
    symmetrised, weights exact multiples of 1/16"""
    exe = os.path.join(REPO, "tools", "hipmcl_check")
    if not os.path.exists(exe):
        pytest.fail("tools/hipmcl_check is not built (make -C combblas-spmm-test_amd drivers)")
    a = cbg.rmat_tile(10, 16).to_host()
    r, c = a["ir"].astype(np.int64), hr.cols_of(a)
    key = np.unique(np.concatenate([r * 1024 + c, c * 1024 + r]))
    r, c = key // 1024, key % 1024
    w = (1 + (7 * np.minimum(r, c) + 13 * np.maximum(r, c)) % 8) / 16.0
    t = hr.from_coo(1024, 1024, r, c, w)
    ps = (2.0, 1e-4, 30, 40, 0.9)
    labels, its = cbg.HipMCL(_mat(cbg, grid, t), inflation=ps[0], prunelimit=ps[1], select=ps[2], recover_num=ps[3],
                             recover_pct=ps[4])
    assert 1 < labels.max() + 1 < 1024 and cbg.hipmcl_stats()["chaos"] <= hr.EPS
    mtx = str(tmp_path / "a.mtx")
    cbg.write_mm(mtx, t)
    run = subprocess.run([exe, mtx] + [repr(x) if isinstance(x, float) else str(x) for x in ps], capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0 and "HIPMCLCHECK OK" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"iterations {its}\n" in run.stdout, (its, run.stdout[-1500:])
    assert f"clusters {labels.max() + 1} labels {_fnv1a_labels(labels)}" in run.stdout, run.stdout[-1500:]


def test_write_clusters(cbg, tmp_path):
    p = tmp_path / "c.txt"
    cbg.write_clusters(str(p), [0, 1, 0, 2, 1])
    assert p.read_text() == "0 2\n1 4\n3\n"


# ---------------------------------------------------------------------------
# several ranks on one GPU
# ---------------------------------------------------------------------------
def _launch(nproc, args, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(HERE, "hipmcl_worker.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = r.stdout + r.stderr
    errs = [ln for ln in out.splitlines() if "CbgError" in ln or "[cbg]" in ln or "AssertionError" in ln]
    return r.returncode, "\n".join(errs[:16]) + "\n" + out


@pytest.mark.parametrize("grid_shape", [(2, 1), (1, 2), (2, 2)])
def test_hipmcl_multirank_host_transport(grid_shape):
    """every operation's gathered result has the bits of the 1 x 1 result (tests/hipmcl_worker.py
    says where the fused inflation cannot); HipMCL on the planted and the hub case gives the
    1 x 1 partition and iteration count"""
    rc, out = _launch(grid_shape[0] * grid_shape[1], ["gpu", str(grid_shape[0]), str(grid_shape[1])])
    assert rc == 0 and out.count("HIPMCLOK") == grid_shape[0] * grid_shape[1], out[:1500] + out[-3000:]


def test_hipmcl_multirank_rccl():
    rc, out = _launch(2, ["rccl", "2", "1"])
    assert rc == 0 and out.count("HIPMCLOK") == 2 and "transport rccl" in out, out[:1500] + out[-3000:]
