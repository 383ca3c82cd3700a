"""The restatements of tests/betwcent_ref.py against the fixtures and hand-made cases, the new
symbols of the library, and every argument check of the new entry points that precedes device
work (no GPU needed)."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import betwcent_ref as br
import hipmcl_ref as hr
from betwcent_worker import CASES, bound, load_case
from test_hipmcl_cpu import _self_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------
# the element-wise restatement
# ---------------------------------------------------------------------------
def _dense(t):
    d = np.zeros((t["m"], t["n"]))
    d[t["ir"], hr.cols_of(t)] = t["val"]
    return d


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_ewise_restatement_equals_dense(seed):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(1, 40)), int(rng.integers(1, 40))

    def make():
        keep = rng.random((m, n)) < 0.35
        r, c = np.nonzero(keep)
        return (hr.from_coo(m, n, r, c, rng.integers(1, 9, len(r)).astype(float)) if len(r) else br.empty(m, n)), keep

    (a, _), (b, kb) = make(), make()
    np.testing.assert_array_equal(_dense(br.ewise(a, b, br.MULT)), _dense(a) * _dense(b))
    np.testing.assert_array_equal(_dense(br.ewise(a, b, br.FIRST)), _dense(a) * kb)
    np.testing.assert_array_equal(_dense(br.ewise(a, b, br.EXCLUDE)), _dense(a) * ~kb)
    for op in (br.MULT, br.FIRST, br.EXCLUDE):
        got = br.ewise(a, b, op)
        assert len(got["jc"]) == len(np.unique(hr.cols_of(got))) and got["cp"][-1] == len(got["ir"])
        assert np.all(np.diff(got["cp"]) > 0)  # an emptied column leaves jc
    assert len(br.ewise(a, None, br.MULT)["ir"]) == 0 and len(br.ewise(a, br.empty(m, n), br.FIRST)["ir"]) == 0
    np.testing.assert_array_equal(_dense(br.ewise(a, None, br.EXCLUDE)), _dense(a))


def test_ewise_restatement_keeps_bits_and_stored_zeros():
    nan = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]
    a = hr.from_coo(6, 2, [0, 1, 2, 3], [0, 0, 0, 1], [-0.0, 0.0, nan, np.inf])
    b = hr.from_coo(6, 2, [0, 2, 5], [0, 0, 1], [0.0, 1.0, 1.0])
    first, excl = br.ewise(a, b, br.FIRST), br.ewise(a, b, br.EXCLUDE)
    assert first["val"].view(np.uint64).tolist() == [0x8000000000000000, 0x7FF8000000ABCDEF]
    assert excl["ir"].tolist() == [1, 3] and excl["jc"].tolist() == [0, 1] and excl["val"].tolist() == [0.0, np.inf]
    mult = br.ewise(a, b, br.MULT)
    assert mult["ir"].tolist() == [0, 2] and np.signbit(mult["val"][0]) and np.isnan(mult["val"][1])


def test_ewise_classes():
    a = hr.from_coo(100, 3, list(range(0, 20, 2)) + [5], [0] * 10 + [2], np.ones(11))
    b = hr.from_coo(100, 3, list(range(0, 30)) + [7], [0] * 30 + [1], np.ones(31))
    # chunks of 4 entries of a: rows 0..6, 8..14, 16..18 span 7, 7 and 3 rows of b; column 2 is not in b
    assert br.ewise_classes(a, b, 4, 7) == (4, 1, 3, 0)
    assert br.ewise_classes(a, b, 4, 6) == (4, 1, 1, 2)
    assert br.ewise_classes(a, b, 16, 18) == (2, 1, 0, 1)


# ---------------------------------------------------------------------------
# the exact Brandes
# ---------------------------------------------------------------------------
def test_brandes_path_and_star():
    # a directed path 0 -> 1 -> 2 -> 3: from root 0, vertex 1 lies on the paths to 2 and 3, vertex 2 on one
    path = hr.from_coo(4, 4, [0, 1, 2], [1, 2, 3], np.ones(3))
    r = br.brandes(path, [0])
    assert r["bc"] == [0, 2, 1, 0] and r["depth"] == [3] and r["levels"] == [[1, 1, 1]] and r["sigma"] == [[1, 1, 1, 1]]
    assert br.brandes(path, [0, 1, 2, 3])["bc"] == [0, 2, 2, 0]
    assert br.brandes(path, [3])["bc"] == [0, 0, 0, 0] and br.brandes(path, [3])["levels"] == [[]]
    # an undirected star: every pair of leaves goes through the centre
    k = 5
    star = hr.from_coo(k + 1, k + 1, [0] * k + list(range(1, k + 1)), list(range(1, k + 1)) + [0] * k, np.ones(2 * k))
    assert br.brandes(star, list(range(k + 1)))["bc"] == [k * (k - 1)] + [0] * k
    # a diamond 0 -> {1, 2} -> 3: two shortest paths, half a dependency each; a loop changes nothing
    dia = hr.from_coo(4, 4, [0, 0, 1, 2, 1], [1, 2, 3, 3, 1], np.ones(5))
    r = br.brandes(dia, [0])
    assert r["bc"] == [0, Fraction(1, 2), Fraction(1, 2), 0] and r["sigma_max"] == 2 and r["levels"] == [[2, 1]]
    assert br.brandes(dia, [0, 1], batch=1)["levels"] == [[2, 1], [1]]
    assert br.brandes(dia, [0, 1], batch=2)["levels"] == [[3, 1]]
    assert br.max_degree(dia) == 2 and br.bound_factor(2, 2, 1, 1) == 16


def test_fixtures_present():
    for name in CASES:
        assert os.path.exists(os.path.join(GOLDEN, f"betwcent_{name}.npz")), name


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference(name):
    """the exact values are the fixture's, and the reference's own run is within the bound of them"""
    z, a, at = load_case(name)
    assert not np.any(z["row"] == z["col"])
    for key in ("cp", "jc", "ir"):  # AT is A's transpose
        np.testing.assert_array_equal(hr.from_coo(a["n"], a["n"], hr.cols_of(a), a["ir"], a["val"])[key], at[key])
    ex = br.brandes(a, z["roots"].tolist(), int(z["batch"]))
    assert [float(x) for x in ex["bc"]] == z["bc_exact"].tolist()
    assert max(ex["depth"]) == int(z["depth"]) and br.max_degree(a) == int(z["degree"])
    assert ex["sigma_max"] == int(z["sigma_max"]) < 2 ** 31
    assert [x for lv in ex["levels"] for x in lv] == z["level_sizes"].tolist()
    assert [len(lv) for lv in ex["levels"]] == z["level_counts"].tolist()
    nref = len(z["ref_roots"])
    assert br.brandes(a, z["ref_roots"].tolist())["bc"] == ex["bc"]  # an isolated root adds nothing
    outdeg = np.bincount(z["row"], minlength=a["n"])
    np.testing.assert_array_equal(z["ref_roots"], np.flatnonzero(outdeg > 0)[:nref])  # the reference's rule
    bnd = bound(z, nref, -(-nref // int(z["batch"])))
    assert np.all(np.abs(z["bc_ref"] - z["bc_exact"]) <= bnd)
    assert 1.0 / float(z["sigma_max"]) > 1e-7 > bnd.max()  # a lost path would show
    if name == "lattice":
        assert int(z["sigma_max"]) == 705432  # C(22, 11)
    if name == "components":
        assert z["roots"][0] == 0 and outdeg[0] == 0 and not np.any(z["col"] == 0)  # an isolated root
        assert {1, 2} <= set(z["roots"].tolist()) and z["bc_exact"][1] == z["bc_exact"][2] == 0.0


# ---------------------------------------------------------------------------
# the library, without a device
# ---------------------------------------------------------------------------
def test_symbols_exported(cbg):
    L = cbg.lib()
    for name in ("cbg_tile_ewise", "cbg_ewise_bounds", "cbg_last_ewise_stats", "cbg_grid_betwcent",
                 "cbg_last_betwcent_stats"):
        assert hasattr(L, name), name
    assert (cbg.EWISE_MULT, cbg.EWISE_FIRST, cbg.EWISE_EXCLUDE) == (0, 1, 2)
    assert (cbg.APPLY_POW, cbg.APPLY_SET, cbg.APPLY_RDIV) == (0, 1, 2)
    for name in ("EWiseMult", "SetDifference", "BetwCent", "betwcent_candidates", "ewise_bounds", "ewise_stats",
                 "betwcent_stats"):
        assert callable(getattr(cbg, name)), name
    assert callable(cbg.Tile.ewise)


def test_bounds_and_stats_shape(cbg):
    assert cbg.ewise_bounds() == [512, 1280]
    assert set(cbg.ewise_stats()) == {"entries_a", "entries_b", "entries_out", "units", "units_none", "units_lds",
                                      "units_global", "ms"}
    assert set(cbg.betwcent_stats()) == {"batches", "levels", "deepest", "fringe_entries", "ms_forward", "ms_ewise",
                                         "ms_backward", "ms_dense", "ms_total"}
    assert cbg.lib().cbg_last_ewise_stats(None, 0, None) == 7 and cbg.lib().cbg_last_betwcent_stats(None, 0, None) == 4


def test_capi_argument_errors(cbg):
    L = cbg.lib()
    bad = cbg.INVALIDPARAMS
    dev = cbg.CTile(4, 5, 0, 0, None, None, None, None, 1, 0)   # an (empty) device tile
    wide = cbg.CTile(4, 6, 0, 0, None, None, None, None, 1, 0)
    tall = cbg.CTile(5, 5, 0, 0, None, None, None, None, 1, 0)
    host = cbg.CTile(4, 5, 0, 0, None, None, None, None, 0, 0)
    huge = cbg.CTile((1 << 31) - 1, 5, 0, 0, None, None, None, None, 1, 0)
    out = cbg.CTile()
    D, O = ctypes.byref(dev), ctypes.byref(out)
    # cbg_tile_ewise
    for op in (-1, 3, 1 << 20):
        assert L.cbg_tile_ewise(D, D, op, O) == bad
    assert L.cbg_tile_ewise(None, D, 0, O) == bad
    assert L.cbg_tile_ewise(D, D, 0, None) == bad
    assert L.cbg_tile_ewise(ctypes.byref(host), D, 0, O) == bad
    assert L.cbg_tile_ewise(D, ctypes.byref(host), 0, O) == bad
    assert L.cbg_tile_ewise(ctypes.byref(huge), ctypes.byref(huge), 0, O) == bad
    assert L.cbg_tile_ewise(D, ctypes.byref(wide), 0, O) == cbg.DIMMISMATCH
    assert L.cbg_tile_ewise(D, ctypes.byref(tall), 2, O) == cbg.DIMMISMATCH
    assert b"shape" in L.cbg_last_error()
    # cbg_tile_apply: the new functors are ops 1 and 2, nothing beyond
    for op in (-1, 3, 4):
        assert L.cbg_tile_apply(D, op, 2.0) == bad
    for op in (cbg.APPLY_POW, cbg.APPLY_SET, cbg.APPLY_RDIV):
        assert L.cbg_tile_apply(D, op, float("nan")) == bad
        assert L.cbg_tile_apply(None, op, 1.0) == bad
    for op in (cbg.APPLY_SET, cbg.APPLY_RDIV):  # a tile struct without arrays is no tile for the functors that write val
        assert L.cbg_tile_apply(D, op, 1.0) == bad and b"no arrays" in L.cbg_last_error()
    A = cbg.SpParMat(cbg.Tile(dev), None, 4, 5)
    for op in ("exp", "divide", 3, None, 1.0):
        with pytest.raises(cbg.CbgError) as e:
            A.Apply(op, 2.0)
        assert e.value.code == bad
    with pytest.raises(cbg.CbgError) as e:
        A.tile.ewise(A.tile, "divide")
    assert e.value.code == bad
    A.tile.c = cbg.CTile()  # nothing to free
    # cbg_grid_betwcent
    g = _self_grid(cbg)
    sq = cbg.CTile(6, 6, 0, 0, None, None, None, None, 1, 0)
    S = ctypes.byref(sq)
    roots = np.array([0, 3, 5, 3, 6, -1], np.int64)
    at = lambda k: roots.ctypes.data + 8 * k  # noqa: E731
    bc = np.zeros(6)
    fn = cbg.BETWCENT_LEVEL_FN()

    def call(grid=g.h, A=S, AT=None, gn=6, r=at(0), n=3, p=(2, 0, 0), out=bc.ctypes.data):
        prm = cbg.CBetwcentParams(*p) if p is not None else None
        return L.cbg_grid_betwcent(grid, A, AT, gn, r, n, ctypes.byref(prm) if prm is not None else None, fn, None, out)

    assert call(grid=None) == bad
    assert call(A=None) == bad
    assert call(A=ctypes.byref(host)) == bad
    assert call(AT=ctypes.byref(host)) == bad
    assert call(p=None) == bad
    assert call(gn=-1) == bad
    assert call(n=-1) == bad
    assert call(r=None) == bad
    assert call(out=None) == bad
    assert call(n=4) == bad               # vertex 3 twice
    assert b"distinct" in L.cbg_last_error()
    assert call(r=at(2), n=3) == bad      # vertex 6 of 6
    assert call(r=at(5), n=1) == bad      # vertex -1
    for p in ((0, 0, 0), (-4, 0, 0), (2, 2, 0), (2, 0, 2), (2, -1, 0)):
        assert call(p=p) == bad
    assert np.all(bc == 0.0)
    # a batch with fewer roots than the grid has columns: refused before any device work, the code agreed
    class Two:  # the host transport of rank 0 of two ranks that always agree with it
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return bytes(data) * (2 if comm in (0, 1) else 1)

    g2 = cbg.CommGrid(0, 2, 1, 2, transport="host", host_comm=Two())
    half = ctypes.byref(cbg.CTile(6, 3, 0, 0, None, None, None, None, 1, 0))
    for n, batch in ((1, 4), (3, 2), (1, 1)):  # one root; a last batch of one root
        assert call(grid=g2.h, A=half, AT=half, n=n, p=(batch, 0, 0)) == bad
        assert b"fewer roots" in L.cbg_last_error()
    assert call(grid=g2.h, A=half, AT=None, n=2, p=(2, 0, 0)) == cbg.NOTSQUARE  # 1 x 2 without AT
    assert call(n=1, p=(4, 0, 0), r=at(4)) == bad and b"distinct" in L.cbg_last_error()  # 1 x 1: only the root is bad
    g2.destroy()
    M = cbg.SpParMat(cbg.Tile(sq), g, 6, 6)
    with pytest.raises(cbg.CbgError) as e:
        cbg.BetwCent(M, [1, 1], 2)
    assert e.value.code == bad
    with pytest.raises(cbg.CbgError) as e:
        cbg.BetwCent(cbg.SpParMat(cbg.Tile(dev), g, 4, 5), [1], 2)
    assert e.value.code == cbg.DIMMISMATCH
    with pytest.raises(cbg.CbgError) as e:
        cbg.EWiseMult(M, cbg.SpParMat(cbg.Tile(dev), g, 4, 5))
    assert e.value.code == cbg.DIMMISMATCH
    with pytest.raises(cbg.CbgError) as e:
        cbg.SetDifference(M, cbg.SpParMat(cbg.Tile(sq), _self_grid(cbg), 6, 6))
    assert e.value.code == cbg.GRIDMISMATCH
    g.destroy()
