"""The sparse-indexing restatement (tests/spref_ref.py) on the host, cbg_rand_perm (computed on
the host), and every argument check of the new entry points that precedes device work."""
import ctypes
import os

import numpy as np
import pytest

import hipmcl_ref as hr
import spref_ref as sr
from test_hipmcl_cpu import _self_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_dense_indexing(seed):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    keep = rng.random((m, n)) < 0.3
    row, col = np.nonzero(keep)
    t = hr.from_coo(m, n, row, col, np.arange(1, len(row) + 1.0))  # distinct nonzero values
    d = sr.dense(t)
    for ri, ci in ((rng.permutation(m), rng.permutation(n)), (rng.integers(0, m, 2 * m), rng.integers(0, n, 3)),
                   (np.sort(rng.choice(m, (m + 1) // 2, replace=False)), None), (None, rng.integers(0, n, n + 5)),
                   (np.zeros(0, np.int64), None), (None, None)):
        got = sr.spref(t, ri, ci)
        rr = np.arange(m) if ri is None else ri
        cc = np.arange(n) if ci is None else ci
        np.testing.assert_array_equal(sr.dense(got), d[np.ix_(rr, cc)])
        assert (got["m"], got["n"]) == (len(rr), len(cc)) and np.count_nonzero(d[np.ix_(rr, cc)]) == len(got["ir"])
        col_of = hr.cols_of(got)
        assert np.all((np.diff(got["ir"]) > 0) | (np.diff(col_of) > 0))  # rows ascending in every column


def test_restatement_keeps_value_bits():
    t = sr.main_tile()
    v = t["val"].view(np.uint64)
    assert np.any(v == np.uint64(0x8000000000000000)) and np.any(v == np.uint64(0x7FF8000000ABCDEF)) and np.any(np.isinf(t["val"]))
    ri, ci = sr.index_cases(t["m"], t["n"])["repeats"]
    got = sr.spref(t, ri, ci)
    assert set(got["val"].view(np.uint64).tolist()) <= set(v.tolist())
    assert np.any(got["val"].view(np.uint64) == np.uint64(0x7FF8000000ABCDEF))
    empty_rows = np.setdiff1d(np.arange(t["m"]), t["ir"])
    assert len(empty_rows) == 4 and len(np.setdiff1d(np.arange(t["n"]), t["jc"])) == 4
    assert np.diff(t["cp"]).max() == t["m"] - 4  # the column that holds every live row


def test_fixtures_present():
    for name in sr.GOLDEN_CASES:
        assert os.path.exists(os.path.join(GOLDEN, f"spref_{name}.npz")), name


@pytest.mark.parametrize("case", sr.GOLDEN_CASES)
def test_restatement_equals_reference(case):
    z = np.load(os.path.join(GOLDEN, f"spref_{case}.npz"), allow_pickle=False)
    t, ri, ci = sr.golden_case(case)
    zin = hr.from_coo(int(z["m"]), int(z["n"]), z["in_row"], z["in_col"], z["in_val"])
    for key in ("cp", "jc", "ir"):
        np.testing.assert_array_equal(t[key], zin[key])
    np.testing.assert_array_equal(t["val"].view(np.uint64), zin["val"].view(np.uint64))
    np.testing.assert_array_equal(ri, z["ri"])
    np.testing.assert_array_equal(ci, z["ci"])
    got = sr.spref(t, ri, ci)
    np.testing.assert_array_equal(got["ir"], z["out_row"])
    np.testing.assert_array_equal(hr.cols_of(got), z["out_col"])
    np.testing.assert_array_equal(got["val"].view(np.uint64), z["out_val"].view(np.uint64))


def test_rand_perm_restatement():
    for n in (0, 1, 2, 97, 4096):
        p = sr.rand_perm(n, 1)
        np.testing.assert_array_equal(np.sort(p), np.arange(n))
        np.testing.assert_array_equal(p, sr.rand_perm(n, 1))  # fixed for a seed
    assert not np.array_equal(sr.rand_perm(97, 1), sr.rand_perm(97, 2))
    assert not np.array_equal(sr.rand_perm(97, 1), np.arange(97))
    np.testing.assert_array_equal(sr.rand_perm(6, 1), [int(x) for x in sr.rand_perm(6, 1)])


def test_cbg_rand_perm_equals_restatement(cbg):
    for n, seed in ((0, 1), (1, 1), (97, 1), (5000, 0x5EED), (5000, 2 ** 63 + 5)):
        np.testing.assert_array_equal(cbg.rand_perm(n, seed), sr.rand_perm(n, seed))
    assert cbg.lib().cbg_rand_perm(-1, 1, None) == cbg.INVALIDPARAMS
    assert cbg.lib().cbg_rand_perm(3, 1, None) == cbg.INVALIDPARAMS


def test_load_imbalance_restatement():
    t = hr.from_coo(8, 8, [0, 1, 2, 3], [0, 1, 2, 3], np.ones(4))
    assert sr.load_imbalance(t, 1, 1) == 1.0 and sr.load_imbalance(t, 2, 2) == 4.0 and sr.load_imbalance(t, 2, 1) == 2.0
    d = hr.from_coo(8, 8, np.arange(8), np.arange(8), np.ones(8))
    assert sr.load_imbalance(d, 2, 2) == 2.0


def test_prepared_restatement():
    """what the GPU tests rely on: RandPermute keeps the partition and the iteration count of both
    cases; RemoveIsolated keeps them where no vertex has in-edges only (planted) and changes them
    where some do (hub)"""
    for case in sorted(hr.CASES):
        t = hr.CASES[case]()
        for ps in hr.PARAM_SETS:
            lab, it, _, _ = hr.hipmcl(t, *ps)
            assert it == (12 if ps[0] == 2.0 else 14)
            plab, pit, _, ids = sr.hipmcl_prepared(t, ps, randpermute=True, seed=1)
            assert pit == it and np.array_equal(plab, lab) and np.array_equal(ids, sr.rand_perm(t["n"], 1))
            g = sr.pad_isolated(t, sr.pad_positions(t["n"]))
            ulab, uit, _, _ = hr.hipmcl(g, *ps)
            rlab, rit, _, rid = sr.hipmcl_prepared(g, ps, remove_isolated=True)
            if case == "planted":
                assert rit == uit and np.array_equal(rlab, ulab) and len(rid) == t["n"] - 2
            else:
                assert len(rid) == 52 and rit == (10 if ps[0] == 2.0 else 11) and not np.array_equal(rlab, ulab)


def test_capi_argument_errors(cbg):
    L = cbg.lib()
    dev = cbg.CTile(4, 5, 0, 0, None, None, None, None, 1, 0)   # an (empty) device tile
    sq = cbg.CTile(4, 4, 0, 0, None, None, None, None, 1, 0)
    host = cbg.CTile(4, 5, 0, 0, None, None, None, None, 0, 0)
    out = cbg.CTile()
    bad = cbg.INVALIDPARAMS
    D, S, O = ctypes.byref(dev), ctypes.byref(sq), ctypes.byref(out)
    idx = np.array([0, 3, 4, -1, 5], np.int64)
    at = lambda k: idx.ctypes.data + 8 * k  # noqa: E731
    # one tile
    assert L.cbg_tile_spref(None, None, 0, None, 0, O) == bad
    assert L.cbg_tile_spref(ctypes.byref(host), None, 0, None, 0, O) == bad
    assert L.cbg_tile_spref(D, None, 0, None, 0, None) == bad
    assert L.cbg_tile_spref(D, at(0), -1, None, 0, O) == bad
    assert L.cbg_tile_spref(D, None, 0, at(0), -1, O) == bad
    assert L.cbg_tile_spref(D, at(2), 1, None, 0, O) == bad      # row 4 of 4 rows
    assert L.cbg_tile_spref(D, at(3), 1, None, 0, O) == bad      # row -1
    assert L.cbg_tile_spref(D, None, 0, at(4), 1, O) == bad      # column 5 of 5 columns
    assert L.cbg_tile_spref(D, at(0), 2, at(3), 1, O) == bad     # column -1
    assert b"index" in L.cbg_last_error()
    # the grid
    assert L.cbg_grid_spref(None, D, 4, 5, None, 0, None, 0, O) == bad
    g = _self_grid(cbg)
    assert L.cbg_grid_spref(g.h, None, 4, 5, None, 0, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, ctypes.byref(host), 4, 5, None, 0, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, D, 4, 5, None, 0, None, 0, None) == bad
    assert L.cbg_grid_spref(g.h, D, 5, 5, None, 0, None, 0, O) == bad    # gm does not fit the tile
    assert L.cbg_grid_spref(g.h, D, 4, 4, None, 0, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, D, -4, 5, None, 0, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, D, 4, 5, at(0), -1, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, D, 4, 5, at(2), 1, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, D, 4, 5, at(3), 1, None, 0, O) == bad
    assert L.cbg_grid_spref(g.h, D, 4, 5, None, 0, at(4), 1, O) == bad
    assert L.cbg_grid_spref(g.h, D, 4, 5, at(0), 2, at(3), 1, O) == bad
    # HipMCL with the two steps: cbg_grid_hipmcl's checks
    ibuf = (ctypes.c_int64 * 8)()
    nw = ctypes.c_int64()

    def params(inflation=2.0, prune=(1e-4, 8, 10, 0.9), preprune=-1, eps=0.0, max_iterations=0):
        return cbg.CHipMclParams(inflation, cbg.CMclParams(*prune), 1, 0, 0, preprune, 0, eps, max_iterations)

    for prep in (cbg.CHipMclPrep(1, 0, 1), cbg.CHipMclPrep(0, 1, 1), cbg.CHipMclPrep(0, 0, 1)):
        P = ctypes.byref(prep)
        call = lambda grid, tile, gn, p: L.cbg_grid_hipmcl_prepared(  # noqa: E731
            grid, tile, gn, p, P, cbg.HIPMCL_ITER_FN(), None, None, ibuf, None, None, ibuf, ctypes.byref(nw))
        assert call(None, S, 4, ctypes.byref(params())) == bad
        assert call(g.h, None, 4, ctypes.byref(params())) == bad
        assert call(g.h, S, 4, None) == bad
        assert call(g.h, S, -1, ctypes.byref(params())) == bad
        for p in (params(inflation=float("nan")), params(inflation=-2.0), params(max_iterations=-1),
                  params(prune=(1e-4, -1, 0, 0.9)), params(preprune=2), params(eps=float("nan"))):
            assert call(g.h, S, 4, ctypes.byref(p)) == bad
    assert L.cbg_grid_nonisolated(None, S, 4, ibuf, ctypes.byref(nw)) == bad
    assert L.cbg_grid_nonisolated(g.h, S, 4, None, ctypes.byref(nw)) == bad
    assert L.cbg_grid_nonisolated(g.h, S, 4, ibuf, None) == bad
    assert L.cbg_grid_nonisolated(g.h, S, -1, ibuf, ctypes.byref(nw)) == bad
    g.destroy()


def test_bounds_and_stats_shape(cbg):
    assert cbg.spref_sort_bounds() == [256, 2048]
    assert set(cbg.spref_stats()) == {"entries_in", "entries_out", "sorted_wave", "sorted_lds", "sorted_radix",
                                      "cols_monotone", "bytes_recv", "ms_col", "ms_row", "ms_sort"}
