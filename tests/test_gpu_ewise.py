"""cbg_tile_ewise (csrc/cbg_ewise.hip) against the NumPy restatement (tests/betwcent_ref.py): the
structure exactly, the values by bits (under MULT a NaN by position).  The shapes sit on the
op's two bounds, C entries of a per work unit and L row ids of b matched in LDS, and the class
counts of cbg_last_ewise_stats prove which matching ran.  Also the two Apply functors that come
with it, and EWiseMult / SetDifference of the Python mirror.

The largest local dimension the C ABI takes is 2^31 - 2 (every entry point refuses more), so the
tile that pins the 64-bit range bound has m = 2^31 - 2 and entries at rows 0 and 2^31 - 3; that
m = 2^31 - 1 is refused is asserted beside it."""
import ctypes
import functools

import numpy as np
import pytest

import betwcent_ref as br
import hipmcl_ref as hr
from helpers import assert_tiles_bits_equal
from test_gpu_hipmcl import _self_grid

pytestmark = pytest.mark.gpu
C, L = 512, 1280
OPS = (("mult", br.MULT), ("first", br.FIRST), ("exclude", br.EXCLUDE))
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]


def test_bounds(cbg):
    assert cbg.ewise_bounds() == [C, L]


def _tile(m, n, cols):
    """cols: {column: (rows, values)}"""
    row = np.concatenate([np.asarray(cols[j][0], np.int64) for j in sorted(cols)] or [np.zeros(0, np.int64)])
    col = np.concatenate([np.full(len(cols[j][0]), j, np.int64) for j in sorted(cols)] or [np.zeros(0, np.int64)])
    val = np.concatenate([np.asarray(cols[j][1], np.float64) for j in sorted(cols)] or [np.zeros(0)])
    return hr.from_coo(m, n, row, col, val) if len(row) else br.empty(m, n)


def _vals(rng, k):
    return rng.integers(1, 1 << 20, k) / 64.0 * rng.choice([-1.0, 1.0], k)


M, N = 9000, 24
LENGTHS = {1: 1, 3: C - 1, 5: C, 8: C + 1, 11: 3 * C + 7, 20: 130}


@functools.lru_cache(maxsize=None)
def _a():
    """columns of 1, C - 1, C, C + 1 and 3C + 7 entries (and a short one) at even rows of [3000, 7000)"""
    rng = np.random.default_rng(7)
    cols = {}
    for j, ln in LENGTHS.items():
        rows = 3000 + 2 * np.sort(rng.choice(2000, ln, replace=False))
        cols[j] = (rows, _vals(rng, ln))
    return _tile(M, N, cols)


@functools.lru_cache(maxsize=None)
def _b(kind):
    rng = np.random.default_rng(11)
    a = _a()
    cols = {}
    for p, j in enumerate(a["jc"].tolist()):
        rows = a["ir"][a["cp"][p]:a["cp"][p + 1]].astype(np.int64)
        if kind == "absent":       # b stores other columns only
            cols[j + 1] = (rows, _vals(rng, len(rows)))
        elif kind == "below":      # every row of b under a's first
            r = np.sort(rng.choice(3000, min(len(rows), 900), replace=False))
            cols[j] = (r, _vals(rng, len(r)))
        elif kind == "above":
            r = 7000 + np.sort(rng.choice(2000, min(len(rows), 900), replace=False))
            cols[j] = (r, _vals(rng, len(r)))
        elif kind == "identical":
            cols[j] = (rows, _vals(rng, len(rows)))
        elif kind == "interleaved":  # the odd rows between a's even ones: ranges, and not one hit
            cols[j] = (rows[:-1] + 1 if len(rows) > 1 else rows + 1, _vals(rng, max(len(rows) - 1, 1)))
        elif kind == "half":       # every other entry of a, and strangers between
            r = np.union1d(rows[::2], 3001 + 2 * rng.choice(2000, len(rows) // 3, replace=False))
            cols[j] = (r, _vals(rng, len(r)))
        elif kind == "dense":      # every row of [2990, 7010): the longest column's ranges pass L
            r = np.arange(2990, 7010)
            cols[j] = (r, _vals(rng, len(r)))
        elif kind == "some_columns" and j in (3, 11):
            cols[j] = (rows[1:], _vals(rng, len(rows) - 1))
    return _tile(M, N, cols)


KINDS = ("absent", "below", "above", "identical", "interleaved", "half", "dense", "some_columns")


def _check(cbg, a, b, A, B):
    for name, code in OPS:
        want = br.ewise(a, b, code)
        T = A.ewise(B, name)
        st = cbg.ewise_stats()
        assert T.digest()["unsorted"] == 0, name
        got = T.to_host()
        assert_tiles_bits_equal(got, want)
        if code != br.MULT:  # a's values, NaN payloads included
            np.testing.assert_array_equal(got["val"].view(np.uint64), want["val"].view(np.uint64))
        assert (st["entries_a"], st["entries_b"], st["entries_out"]) == (len(a["ir"]), len(b["ir"]) if b else 0,
                                                                       len(want["ir"])), (name, st)
        if b is not None and len(b["ir"]) and len(a["ir"]):
            cls = br.ewise_classes(a, b, C, L)
            assert (st["units"], st["units_none"], st["units_lds"], st["units_global"]) == cls, (name, st, cls)
        else:
            assert st["units"] == 0, st
        T.free()


@pytest.mark.parametrize("kind", KINDS)
def test_ewise_bits(cbg, kind):
    a, b = _a(), _b(kind)
    A, B = cbg.Tile.from_dict(a), cbg.Tile.from_dict(b)
    _check(cbg, a, b, A, B)
    cls = br.ewise_classes(a, b, C, L)
    assert cls[0] == 1 + 1 + 1 + 2 + 4 + 1  # the units of columns of 1, C - 1, C, C + 1, 3C + 7 and 130 entries
    if kind in ("absent", "below", "above"):
        assert cls[1] == cls[0]
    if kind in ("identical", "half"):
        assert cls[2] == cls[0]
    if kind == "interleaved":
        # the one-entry column and the one-entry chunk of the C + 1 column have nothing of b in their rows
        assert cls[1] == 2 and cls[2] == cls[0] - 2 and br.ewise(a, b, br.MULT)["cp"][-1] == 0  # every column emptied
    if kind == "dense":
        assert cls[3] >= 4 and cls[2] >= 2  # both matchings ran in one call


def test_ewise_empty_and_null(cbg):
    a = _a()
    A, E = cbg.Tile.from_dict(a), cbg.Tile.from_dict(br.empty(M, N))
    _check(cbg, a, None, A, None)
    _check(cbg, a, br.empty(M, N), A, E)
    _check(cbg, br.empty(M, N), a, E, A)
    _check(cbg, br.empty(M, N), br.empty(M, N), E, E)
    X = A.ewise(None, "exclude")
    assert_tiles_bits_equal(X.to_host(), a)
    assert A.ewise(E, "mult").nnz == 0 and A.ewise(None, "first").nzc == 0


def test_ewise_lds_bound(cbg):
    """three columns whose only unit spans a range of L - 1, L and L + 1 row ids of b"""
    rng = np.random.default_rng(3)
    acols, bcols = {}, {}
    for j, ln in ((2, L - 1), (5, L), (6, L + 1)):
        acols[j] = ([10, 400, 10 + ln - 1], _vals(rng, 3))
        bcols[j] = (np.arange(10, 10 + ln), _vals(rng, ln))
    a, b = _tile(4000, 9, acols), _tile(4000, 9, bcols)
    assert br.ewise_classes(a, b, C, L) == (3, 0, 2, 1)
    _check(cbg, a, b, cbg.Tile.from_dict(a), cbg.Tile.from_dict(b))
    # the range of a unit is cut at its chunk's last row: the entries of b beyond it do not count
    a2 = _tile(4000, 9, {2: ([10, L + 8], [1.0, 2.0]), 5: ([10, L + 9], [3.0, 4.0]), 6: ([10, L + 10], [5.0, 6.0])})
    b2 = _tile(4000, 9, {j: (np.arange(10, 3000), _vals(rng, 2990)) for j in (2, 5, 6)})
    assert br.ewise_classes(a2, b2, C, L) == (3, 0, 2, 1)
    _check(cbg, a2, b2, cbg.Tile.from_dict(a2), cbg.Tile.from_dict(b2))


def test_ewise_huge_rows(cbg):
    """rows at both ends of the largest tile: the range's upper bound is the last row plus one"""
    m = (1 << 31) - 2
    a = _tile(m, 3, {1: ([0, m - 1], [2.0, 3.0]), 2: ([m - 1], [7.0])})
    b = _tile(m, 3, {1: ([5, m - 1], [10.0, 0.5]), 2: ([m - 2], [1.0])})
    assert br.ewise(a, b, br.MULT)["ir"].tolist() == [m - 1] and br.ewise(a, b, br.MULT)["val"].tolist() == [1.5]
    _check(cbg, a, b, cbg.Tile.from_dict(a), cbg.Tile.from_dict(b))
    with pytest.raises(cbg.CbgError) as e:  # the C ABI's largest dimension
        cbg.Tile.from_dict(dict(a, m=m + 1))
    assert e.value.code == cbg.INVALIDPARAMS


def test_ewise_self(cbg):
    a = _a()
    A = cbg.Tile.from_dict(a)
    _check(cbg, a, a, A, A)
    assert A.ewise(A, "exclude").nnz == 0
    assert_tiles_bits_equal(A.ewise(A, "first").to_host(), a)
    np.testing.assert_array_equal(A.ewise(A, "mult").to_host()["val"], a["val"] * a["val"])


def test_ewise_special_values(cbg):
    inf = np.inf
    av = [-0.0, 0.0, inf, -inf, NAN_PAYLOAD, 1.5, 0.0, inf, -0.0, 3.0]
    a = _tile(40, 4, {0: (np.arange(0, 20, 2), av), 3: ([1, 2, 3], [-0.0, NAN_PAYLOAD, 0.0])})
    # hits at rows 0, 4, 8, 12, 14, 16, 18: 0 * inf, inf * 0 and NaN * 1 among them
    b = _tile(40, 4, {0: ([0, 1, 4, 8, 12, 14, 16, 18], [inf, 1.0, 0.0, 1.0, -0.0, -inf, 2.0, NAN_PAYLOAD]),
                      3: ([2, 3], [1.0, -1.0])})
    A, B = cbg.Tile.from_dict(a), cbg.Tile.from_dict(b)
    _check(cbg, a, b, A, B)
    first, excl = A.ewise(B, "first").to_host(), A.ewise(B, "exclude").to_host()
    bits = np.concatenate([first["val"], excl["val"]]).view(np.uint64)
    assert sorted(bits.tolist()) == sorted(a["val"].view(np.uint64).tolist())  # every value of a, in one or the other
    assert np.uint64(0x7FF8000000ABCDEF) in first["val"].view(np.uint64)
    mult = A.ewise(B, "mult").to_host()
    assert np.isnan(mult["val"][[0, 1, 2]]).all() and mult["val"][3] == 0.0 and np.signbit(mult["val"][3])


def test_ewise_errors(cbg):
    Lb = cbg.lib()
    a, b = cbg.Tile.from_dict(_tile(5, 4, {1: ([2], [1.0])})), cbg.Tile.from_dict(_tile(5, 4, {1: ([2], [1.0])}))
    wide, tall = cbg.Tile.from_dict(br.empty(5, 5)), cbg.Tile.from_dict(br.empty(6, 4))
    out = cbg.CTile()
    A, B, O = ctypes.byref(a.c), ctypes.byref(b.c), ctypes.byref(out)
    assert Lb.cbg_tile_ewise(A, ctypes.byref(wide.c), 0, O) == cbg.DIMMISMATCH
    assert Lb.cbg_tile_ewise(A, ctypes.byref(tall.c), 2, O) == cbg.DIMMISMATCH
    for op in (-1, 3, 99):
        assert Lb.cbg_tile_ewise(A, B, op, O) == cbg.INVALIDPARAMS
    assert Lb.cbg_tile_ewise(None, B, 0, O) == cbg.INVALIDPARAMS
    assert Lb.cbg_tile_ewise(A, B, 0, None) == cbg.INVALIDPARAMS
    with pytest.raises(cbg.CbgError) as e:
        a.ewise(b, "divide")
    assert e.value.code == cbg.INVALIDPARAMS
    assert out.nnz == 0 and not out.cp  # nothing was produced


def test_ewisemult_and_setdifference(cbg):
    g = _self_grid(cbg)
    a, b = _a(), _b("half")
    A = cbg.SpParMat(cbg.Tile.from_dict(a), g, M, N)
    B = cbg.SpParMat(cbg.Tile.from_dict(b), g, M, N)
    assert_tiles_bits_equal(cbg.EWiseMult(A, B, False).tile.to_host(), br.ewise(a, b, br.MULT))
    assert_tiles_bits_equal(cbg.EWiseMult(A, B, True).tile.to_host(), br.ewise(a, b, br.EXCLUDE))
    D = cbg.SetDifference(A, B)
    assert_tiles_bits_equal(D.tile.to_host(), br.ewise(a, b, br.EXCLUDE))
    assert (D.gm, D.gn) == (M, N) and D.grid is g
    # A = (A .* B-mask) + (A \ B): the two parts are disjoint and cover A
    both = cbg.SpParMat(A.tile.ewise(B.tile, "first"), g, M, N)
    both += D
    assert_tiles_bits_equal(both.tile.to_host(), a)
    other = cbg.SpParMat(cbg.Tile.from_dict(br.empty(M, N + 1)), g, M, N + 1)
    with pytest.raises(cbg.CbgError) as e:
        cbg.EWiseMult(A, other)
    assert e.value.code == cbg.DIMMISMATCH
    g2 = _self_grid(cbg)
    with pytest.raises(cbg.CbgError) as e:
        cbg.SetDifference(A, cbg.SpParMat(B.tile, g2, M, N))
    assert e.value.code == cbg.GRIDMISMATCH
    g2.destroy()
    g.destroy()


# ---------------------------------------------------------------------------
# Apply: set, rdiv
# ---------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("nnz", [1, 2, 64, 517])
def test_apply_set_rdiv_bits(cbg, nnz):
    """on a val that starts 8 bytes off a 16-byte boundary too (a borrowed view from the second entry on)"""
    rng = np.random.default_rng(nnz)
    v = rng.uniform(-3.0, 3.0, nnz + 1)
    v[1] = 0.0              # 1 / 0 = inf
    v[-1] = -0.0            # 1 / -0 = -inf
    t = hr.from_coo(nnz + 1, 1, np.arange(nnz + 1), np.zeros(nnz + 1), v)
    for op, arg in ((cbg.APPLY_RDIV, 1.0), (cbg.APPLY_RDIV, -2.5), (cbg.APPLY_SET, 1.0), (cbg.APPLY_SET, -0.0)):
        base = cbg.Tile.from_dict(t)
        view = cbg.CTile(base.c.m, 1, nnz, 1, base.c.cp, base.c.jc, base.c.ir + 4, base.c.val + 8, 1, 0)
        assert cbg.lib().cbg_tile_apply(ctypes.byref(view), op, arg) == 0
        with np.errstate(divide="ignore"):
            tail = arg / v[1:] if op == cbg.APPLY_RDIV else np.full(nnz, arg)
        np.testing.assert_array_equal(_bits(base.to_host()["val"]), _bits(np.concatenate([v[:1], tail])))
    with np.errstate(divide="ignore"):
        assert np.isinf(1.0 / v[1:]).sum() == (2 if nnz > 1 else 1)


def test_apply_mirror(cbg):
    g = _self_grid(cbg)
    a = _a()
    A = cbg.SpParMat(cbg.Tile.from_dict(a), g, M, N)
    A.Apply("rdiv", 1.0)
    np.testing.assert_array_equal(_bits(A.tile.to_host()["val"]), _bits(1.0 / a["val"]))
    A.Apply("set", 1.0)
    np.testing.assert_array_equal(_bits(A.tile.to_host()["val"]), _bits(np.ones(len(a["val"]))))
    A.Apply(cbg.APPLY_SET, 4.0)
    A.Apply(cbg.APPLY_POW, 2.0)
    assert np.all(A.tile.to_host()["val"] == 16.0)
    for op in ("exp", 3, -1, None, True):
        with pytest.raises(cbg.CbgError) as e:
            A.Apply(op, 2.0)
        assert e.value.code == cbg.INVALIDPARAMS
    assert cbg.lib().cbg_tile_apply(ctypes.byref(A.tile.c), 3, 2.0) == cbg.INVALIDPARAMS
    assert cbg.lib().cbg_tile_apply(ctypes.byref(A.tile.c), cbg.APPLY_SET, float("nan")) == cbg.INVALIDPARAMS
    g.destroy()
