"""Markov-clustering pruning without a GPU: the NumPy restatement (tests/mcl_ref.py)
against the reference's own MCLPruneRecoverySelect output (tests/golden/mcl_*.npz,
made by tests/golden/make_mcl_golden.py), and the argument errors of the new C ABI."""
import ctypes
import glob
import os

import numpy as np
import pytest

import mcl_ref
from helpers import GOLDEN, tile_cols

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "mcl_*.npz")))


def test_fixtures_present():
    assert len(FIXTURES) >= 2, "tests/golden/mcl_*.npz missing"


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_restatement_equals_reference(path):
    """structure exactly, values by bits, for every parameter set; and the fixture's
    matrix is the generator's (so the branch coverage asserted there holds for it)"""
    z = np.load(path, allow_pickle=False)
    t = dict(m=int(z["m"]), n=int(z["n"]), cp=z["cp"].astype(np.int64), jc=z["jc"].astype(np.int32),
             ir=z["ir"].astype(np.int32), val=z["val"].astype(np.float64))
    mcl_ref.assert_all_branches(t, [tuple(p) for p in z["params"]])
    assert len(z["params"]) == len(mcl_ref.PARAM_SETS)
    for k, (h, S, R, q) in enumerate(z["params"]):
        got = mcl_ref.mcl_prune_ref(t, float(h), int(S), int(R), float(q))
        np.testing.assert_array_equal(tile_cols(got), z[f"out{k}_col"])
        np.testing.assert_array_equal(got["ir"], z[f"out{k}_row"])
        np.testing.assert_array_equal(got["val"].view(np.uint64), z[f"out{k}_val"].view(np.uint64))
        assert np.all(np.diff(got["cp"]) > 0)  # emptied columns left jc


def test_generators_cover_every_branch():
    mcl_ref.small_case(1)
    took = {}
    t = mcl_ref.small_case(2)
    mcl_ref.mcl_prune_ref(t, mcl_ref.H, mcl_ref.S_NUM, mcl_ref.R_NUM, mcl_ref.Q, took)
    for b in ("recovery", "selection", "recovery_after_selection", "fewer_than_k", "ties_at_kth", "equal_to_h"):
        assert took[b], b


def test_kth_largest_rules():
    assert mcl_ref.kth_largest([3.0, 1.0, 2.0, 2.0], 3) == 2.0
    assert mcl_ref.kth_largest([3.0, 1.0], 5) == 1.0  # fewer than k entries: the smallest
    assert mcl_ref.kth_largest([-0.0, 0.0, -1.0], 1) == 0.0


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def test_capi_argument_errors(cbg):
    """every check that precedes device work; the codes are the reference's INVALIDPARAMS"""
    L = cbg.lib()
    dev = cbg.CTile(4, 4, 0, 0, None, None, None, None, 1, 0)   # an (empty) device tile
    host = cbg.CTile(4, 4, 0, 0, None, None, None, None, 0, 0)
    buf = (ctypes.c_double * 4)()
    ibuf = (ctypes.c_int64 * 4)()
    out = cbg.CTile()
    bad = cbg.INVALIDPARAMS
    assert L.cbg_tile_col_stats(None, buf, 1, ibuf, buf) == bad
    assert L.cbg_tile_col_stats(ctypes.byref(host), buf, 1, ibuf, buf) == bad
    assert L.cbg_tile_col_stats(ctypes.byref(dev), None, 1, ibuf, buf) == bad
    assert L.cbg_tile_col_stats(ctypes.byref(dev), buf, 2, ibuf, buf) == bad
    assert L.cbg_tile_prune_column(None, buf, ctypes.byref(out)) == bad
    assert L.cbg_tile_prune_column(ctypes.byref(dev), buf, None) == bad
    assert L.cbg_tile_prune_column(ctypes.byref(dev), None, ctypes.byref(out)) == bad
    assert L.cbg_grid_kselect(None, ctypes.byref(dev), None, 0, 1, None) == bad
    assert L.cbg_grid_mcl_prune(None, ctypes.byref(dev), None, ctypes.byref(out)) == bad
    assert L.cbg_summa_spgemm_mcl(None, ctypes.byref(dev), ctypes.byref(dev), 4, 4, 0, 0, 0, 1, 0, cbg.PHASE_FN(), None,
                                  ctypes.byref(out), None) == bad
    g = _self_grid(cbg)
    cols = (ctypes.c_int32 * 1)(0)
    assert L.cbg_grid_kselect(g.h, ctypes.byref(dev), cols, 1, 0, buf) == bad      # k < 1
    assert L.cbg_grid_kselect(g.h, ctypes.byref(dev), cols, -1, 1, buf) == bad
    assert L.cbg_grid_kselect(g.h, ctypes.byref(dev), None, 1, 1, buf) == bad
    assert L.cbg_grid_kselect(g.h, ctypes.byref(host), cols, 1, 1, buf) == bad
    for p in (cbg.CMclParams(0.1, -1, 0, 0.0), cbg.CMclParams(0.1, 0, -2, 0.0), cbg.CMclParams(float("nan"), 1, 1, 0.5),
              cbg.CMclParams(0.1, 1, 1, float("nan"))):
        assert L.cbg_grid_mcl_prune(g.h, ctypes.byref(dev), ctypes.byref(p), ctypes.byref(out)) == bad
        assert L.cbg_summa_spgemm_mcl(g.h, ctypes.byref(dev), ctypes.byref(dev), 4, 4, 0, 0, 0, 1, 0, cbg.PHASE_FN(),
                                      None, ctypes.byref(out), ctypes.byref(p)) == bad
        assert b"MCL" in L.cbg_last_error()
    ok = cbg.CMclParams(0.1, 1, 1, 0.5)
    assert L.cbg_grid_mcl_prune(g.h, ctypes.byref(dev), ctypes.byref(ok), None) == bad
    assert L.cbg_summa_spgemm_mcl(g.h, ctypes.byref(dev), ctypes.byref(dev), 4, 4, 0, 0, 0, 1, 0, cbg.PHASE_FN(), None,
                                  None, ctypes.byref(ok)) == bad  # neither C nor a callback
    g.destroy()


def test_bounds_and_stats_shape(cbg):
    b = cbg.mcl_kselect_bounds()
    assert len(b) == 3 and b == sorted(b) and b[0] >= 64
    c = (ctypes.c_int64 * 10)()
    assert cbg.lib().cbg_last_mcl_stats(c, 10, None) == 10
    assert set(cbg.mcl_stats()["kselect"]) == set(cbg.MCL_KSELECT_CLASSES)
