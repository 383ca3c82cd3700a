"""The HipMCL restatement (tests/hipmcl_ref.py) on the host, and every argument check
of the new entry points that precedes device work."""
import ctypes
import os

import numpy as np
import pytest

import hipmcl_ref as hr


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def test_capi_argument_errors(cbg):
    L = cbg.lib()
    dev = cbg.CTile(4, 4, 0, 0, None, None, None, None, 1, 0)   # an (empty) device tile
    rect = cbg.CTile(4, 5, 0, 0, None, None, None, None, 1, 0)
    host = cbg.CTile(4, 4, 0, 0, None, None, None, None, 0, 0)
    buf = (ctypes.c_double * 8)()
    ibuf = (ctypes.c_int64 * 8)()
    out, c = cbg.CTile(), ctypes.c_double()
    bad = cbg.INVALIDPARAMS
    D, O = ctypes.byref(dev), ctypes.byref(out)

    def params(inflation=2.0, prune=(1e-4, 8, 10, 0.9), preprune=-1, eps=0.0, max_iterations=0):
        return cbg.CHipMclParams(inflation, cbg.CMclParams(*prune), 1, 0, 0, preprune, 0, eps, max_iterations)

    ok = params()
    # a NULL grid
    assert L.cbg_grid_reduce_cols(None, D, 0, 0.0, buf) == bad
    assert L.cbg_grid_make_col_stochastic(None, D) == bad
    assert L.cbg_grid_chaos(None, D, ctypes.byref(c)) == bad
    assert L.cbg_grid_inflate(None, D, 2.0, ctypes.byref(c)) == bad
    assert L.cbg_grid_remove_loops(None, D, 4, 4, O, None) == bad
    assert L.cbg_grid_add_loops(None, D, 4, 4, buf, 0, O) == bad
    assert L.cbg_grid_adjust_loops(None, D, 4, 4, O) == bad
    assert L.cbg_grid_connected_components(None, D, 4, ibuf, None) == bad
    assert L.cbg_grid_hipmcl(None, D, 4, ctypes.byref(ok), cbg.HIPMCL_ITER_FN(), None, None, ibuf, None, None) == bad
    assert L.cbg_tile_apply(None, 0, 2.0) == bad
    assert L.cbg_tile_apply(ctypes.byref(host), 0, 2.0) == bad
    assert L.cbg_tile_apply(D, 1, 2.0) == bad
    assert L.cbg_tile_apply(D, 0, float("nan")) == bad
    g = _self_grid(cbg)
    # gm != gn
    assert L.cbg_grid_remove_loops(g.h, ctypes.byref(rect), 4, 5, O, None) == cbg.DIMMISMATCH
    assert L.cbg_grid_add_loops(g.h, ctypes.byref(rect), 4, 5, buf, 0, O) == cbg.DIMMISMATCH
    assert L.cbg_grid_adjust_loops(g.h, ctypes.byref(rect), 4, 5, O) == cbg.DIMMISMATCH
    assert b"square" in L.cbg_last_error()
    assert L.cbg_grid_remove_loops(g.h, D, 4, 4, None, None) == bad
    assert L.cbg_grid_add_loops(g.h, D, 4, 4, None, 0, O) == bad
    assert L.cbg_grid_remove_loops(g.h, ctypes.byref(host), 4, 4, O, None) == bad
    # reductions
    assert L.cbg_grid_reduce_cols(g.h, D, 4, 0.0, buf) == bad
    assert L.cbg_grid_reduce_cols(g.h, D, -1, 0.0, buf) == bad
    assert L.cbg_grid_reduce_cols(g.h, D, 0, float("nan"), buf) == bad
    assert L.cbg_grid_reduce_cols(g.h, D, 0, 0.0, None) == bad
    assert L.cbg_grid_chaos(g.h, D, None) == bad
    # the inflation: NaN, negative, zero, infinite
    for power in (float("nan"), -2.0, 0.0, float("inf")):
        assert L.cbg_grid_inflate(g.h, D, power, ctypes.byref(c)) == bad
        assert L.cbg_grid_hipmcl(g.h, D, 4, ctypes.byref(params(inflation=power)), cbg.HIPMCL_ITER_FN(), None, None,
                                 ibuf, None, None) == bad
        assert b"inflation" in L.cbg_last_error()
    assert L.cbg_grid_inflate(g.h, D, 2.0, None) == bad
    for p in (params(max_iterations=-1), params(prune=(1e-4, -1, 0, 0.9)), params(prune=(float("nan"), 1, 1, 0.9)),
              params(preprune=2), params(eps=float("nan"))):
        assert L.cbg_grid_hipmcl(g.h, D, 4, ctypes.byref(p), cbg.HIPMCL_ITER_FN(), None, None, ibuf, None, None) == bad
    assert L.cbg_grid_hipmcl(g.h, D, 4, None, cbg.HIPMCL_ITER_FN(), None, None, ibuf, None, None) == bad
    assert L.cbg_grid_hipmcl(g.h, D, -1, ctypes.byref(ok), cbg.HIPMCL_ITER_FN(), None, None, ibuf, None, None) == bad
    assert L.cbg_grid_connected_components(g.h, D, -1, ibuf, None) == bad
    g.destroy()


def test_bounds_and_stats_shape(cbg):
    assert cbg.mcl_moment_bounds() == [16, 4096]
    assert set(cbg.hipmcl_stats()) == {"iterations", "chaos", "final_nnz", "ms_expand", "ms_prune", "ms_inflate"}
    assert len(cbg.inflate_stats()["ms"]) == 3


def test_restatement_operations():
    t = hr.from_coo(4, 4, [0, 1, 3, 2, 1], [0, 0, 0, 2, 3], [0.5, 0.25, 0.25, 0.0, -2.0])
    np.testing.assert_array_equal(hr.reduce_cols(t, "sum"), [1.0, 0.0, 0.0, -2.0])
    np.testing.assert_array_equal(hr.reduce_cols(t, "max", 0.0), [0.5, 0.0, 0.0, 0.0])  # folded from the identity
    np.testing.assert_array_equal(hr.reduce_cols(t, "max", -9.0), [0.5, -9.0, 0.0, -2.0])
    np.testing.assert_array_equal(hr.reduce_cols(t, "count", 7.0), [3.0, 7.0, 1.0, 1.0])
    np.testing.assert_array_equal(hr.reduce_cols(t, "sumsq"), [0.375, 0.0, 0.0, 4.0])
    s = hr.make_col_stochastic(t)
    np.testing.assert_array_equal(s["val"], [0.5, 0.25, 0.25, 0.0, 1.0])  # a zero column: DBL_MAX * 0
    assert hr.chaos(s) == (0.5 - 0.375) * 3
    a = hr.adjust_loops(t)
    d = a["val"][hr.cols_of(a) == a["ir"]]
    # column 0: its largest other entry; 1: empty, min(); 2: only a loop, so empty once it is removed; 3: negative
    np.testing.assert_array_equal(d, [0.25, hr.DBL_MIN, hr.DBL_MIN, hr.DBL_MIN])
    assert hr.make_col_stochastic(a)["val"][hr.cols_of(a) == 1][0] == 1.0
    assert hr.remove_loops(t)[1] == 2  # (0, 0) and (2, 2)


def test_restatement_components_are_canonical():
    lab = hr.components(7, [5, 6, 1], [2, 5, 3])
    np.testing.assert_array_equal(lab, [0, 1, 2, 1, 3, 2, 2])
    np.testing.assert_array_equal(hr.canonical([9, 4, 7, 4, 1, 7, 7]), lab)
    np.testing.assert_array_equal(hr.components(0, [], []), [])


@pytest.mark.parametrize("case", sorted(hr.CASES))
def test_restatement_loop_is_robust(case):
    """the end-to-end cases do not sit on a knife edge: weights perturbed by a relative
    1e-12 give the same partition and iteration count (the device multiply's sum order
    differs from the oracle's), and selection and recovery both fire"""
    t = hr.CASES[case]()
    rng = np.random.default_rng(0)
    for ps in hr.PARAM_SETS:
        took = {}
        lab, it, ch, fin = hr.hipmcl(t, *ps, took=took)
        if ps[2] > 0:
            assert took["selection"] and (took["recovery"] or took["recovery_after_selection"])
        assert ch[-1] <= hr.EPS and len(ch) == it
        p = dict(t, val=t["val"] * (1.0 + 1e-12 * rng.uniform(-1, 1, len(t["val"]))))
        lab2, it2, _, _ = hr.hipmcl(p, *ps)
        assert it2 == it
        np.testing.assert_array_equal(lab2, lab)


# ---------------------------------------------------------------------------
# the reference's own run (tests/golden/hipmcl_*.npz, tests/golden/make_hipmcl_golden.py)
# ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# restatement against the reference's dumps, measured here: pow(v, 1.7) 1 ulp (numpy.power
# against the reference's libm), chaos 4.9e-16 relative (sum order); the bounds are twice the
# ulp distance, and for chaos the end-to-end bound of tests/test_gpu_hipmcl.py (ten times
# the larger of this and the device's 9.56e-14)
POW_ULP = 2
CHAOS_RTOL = 9.56e-13


def test_fixtures_present():
    for name in hr.CASES:
        assert os.path.exists(os.path.join(GOLDEN, f"hipmcl_{name}.npz")), name


@pytest.mark.parametrize("case", sorted(hr.CASES))
def test_restatement_equals_reference(case):
    z = hr.load_golden(case)
    t = hr.CASES[case]()
    for key in ("cp", "jc", "ir"):
        np.testing.assert_array_equal(t[key], z[key])
    np.testing.assert_array_equal(t["val"].view(np.uint64), z["val"].view(np.uint64))
    np.testing.assert_array_equal(hr.interpret(t), z["interpret"])
    assert len(z["params"]) == len(hr.PARAM_SETS)
    for k, ps in enumerate(hr.PARAM_SETS):
        assert tuple(z["params"][k]) == ps
        a = hr.adjust_loops(t)
        s = hr.make_col_stochastic(a)
        f = hr.apply_pow(s, ps[0])
        for w, m in (("adjust", a), ("stoch", s), ("inflate", f)):
            np.testing.assert_array_equal(hr.cols_of(m), z[f"{w}{k}_col"])
            np.testing.assert_array_equal(m["ir"], z[f"{w}{k}_row"])
            d = np.abs(m["val"].view(np.int64) - z[f"{w}{k}_val"].view(np.int64)).max()
            exact = w != "inflate" or ps[0] == 2.0  # dyadic weights: the loops and the column sums are exact
            assert d <= (0 if exact else POW_ULP), (w, ps, int(d))
        want = float(z[f"chaos{k}"])
        assert abs(hr.chaos(s) - want) <= CHAOS_RTOL * max(want, hr.EPS)
        lab, it, ch, _ = hr.hipmcl(t, *ps)
        assert it == int(z[f"iterations{k}"])
        np.testing.assert_array_equal(lab, z[f"labels{k}"])  # both canonical
        assert all(hr.printed_agrees(c, p) for c, p in zip(ch, z[f"printed{k}"])), (ch, z[f"printed{k}"])
