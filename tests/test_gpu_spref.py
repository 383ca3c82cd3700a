"""Sparse indexing on device (csrc/cbg_spref.hip, the grid logic in csrc/cbg_grid_algos.cpp):
Tile.spref and SpParMat.SubsRef against the NumPy restatement (tests/spref_ref.py) by bits,
against the reference's own algorithm run on the device (P * A * Q through the SUMMA), and
against the reference's results (tests/golden/spref_*.npz); HipMCL with RemoveIsolated and
RandPermute against the restatement of the loop on the prepared matrices.

No arithmetic touches a value, so every comparison of matrices is by bits (NaN by position,
as assert_tiles_bits_equal does everywhere).

Chaos with RandPermute / RemoveIsolated: compared with hipmcl_ref.hipmcl of the prepared
matrix under test_gpu_hipmcl.CHAOS_RTOL (9.56e-13, ten times the largest device-against-
restatement difference measured for the unprepared cases); the largest difference of the
prepared cases is printed by the tests.

RemoveIsolated follows the reference: nonisov are the vertices whose column sum is > 0
(MCL.cpp:476-486).  Restated on the host (spref_ref.hipmcl_prepared) this gives, for the cases
padded with five empty vertices: planted n_work 94 of 101 (the case has two isolated vertices
of its own), labels and iterations (12, 14) of the run without removal; hub n_work 52 of 133
(76 of its columns are empty; the vertices among them with in-edges only leave with their rows), iterations
10 and 11 where the run without removal takes 12 and 14, and another partition -- the
reference's behaviour for such vertices.  The device is compared with that restatement, and with
the run without removal where the restatement says they agree (planted).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hipmcl_ref as hr
import spref_ref as sr
from helpers import assert_tiles_bits_equal
from test_gpu_hipmcl import CHAOS_RTOL, _fnv1a_labels, _self_grid
from test_multiprocess import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BOUNDS = [256, 2048]
SEEDS = (1, 2, 3, 0x5EED)


@pytest.fixture
def grid(cbg):
    g = _self_grid(cbg)
    yield g
    g.destroy()


def _mat(cbg, g, d):
    return cbg.SpParMat(cbg.Tile.from_dict(d), g, d["m"], d["n"])


@functools.lru_cache(maxsize=None)
def _main():
    t = sr.main_tile()
    return t, sr.index_cases(t["m"], t["n"])


@functools.lru_cache(maxsize=None)
def _want(name):
    t, cases = _main()
    return sr.spref(t, *cases[name])


def _dig(tile):
    """the digest without the value sum (NaN where the tile holds a NaN; the hashes cover the bits)"""
    d = tile.digest()
    d.pop("vsum")
    return d


def _both(cbg, grid, t, ri, ci):
    """Tile.spref and SubsRef on the 1 x 1 grid: sorted, and the same bits"""
    T = cbg.Tile.from_dict(t)
    before = _dig(T)
    a = T.spref(ri, ci)
    st = cbg.spref_stats()
    A = _mat(cbg, grid, t)
    b = A.SubsRef(ri, ci)
    assert a.digest()["unsorted"] == 0 and b.tile.digest()["unsorted"] == 0
    ah = a.to_host()
    assert_tiles_bits_equal(b.tile.to_host(), ah)
    assert _dig(T) == before and _dig(A.tile) == before  # the input is left as it was
    assert (b.gm, b.gn) == (ah["m"], ah["n"])
    return ah, st, cbg.spref_stats()


# ---------------------------------------------------------------------------
# 1. bits against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.index_cases(301, 257)))
def test_spref_bits(cbg, grid, name):
    t, cases = _main()
    ri, ci = cases[name]
    got, st_tile, st_grid = _both(cbg, grid, t, ri, ci)
    want = _want(name)
    assert_tiles_bits_equal(got, want)
    for st in (st_tile, st_grid):
        assert st["entries_in"] == len(t["ir"]) and st["entries_out"] == len(want["ir"]), st
        if name in ("identity", "increasing", "no_rows", "rows_all"):
            assert st["sorted_wave"] + st["sorted_lds"] + st["sorted_radix"] == 0, st  # no column sorted
        if name in ("identity", "increasing"):
            assert st["cols_monotone"] == len(want["jc"]) > 0
    if name == "identity":
        assert_tiles_bits_equal(got, t)
    if name in ("no_rows", "no_cols"):
        assert len(got["ir"]) == 0 and 0 in (got["m"], got["n"])
    if name == "repeats_tall":
        assert got["m"] > t["m"] and len(got["ir"]) > len(t["ir"])
    if name == "perm":  # the column that holds every live row went through the LDS class
        assert st_tile["sorted_lds"] >= 1 and st_tile["sorted_wave"] > 100


def test_spref_inplace_and_call_alias(cbg, grid):
    t, cases = _main()
    ri, ci = cases["rect"]
    A = _mat(cbg, grid, t)
    B = A(ri, ci)
    assert_tiles_bits_equal(B.tile.to_host(), _want("rect"))
    assert A.SubsRef(ri, ci, inplace=True) is A and (A.gm, A.gn) == (203, 97)
    assert_tiles_bits_equal(A.tile.to_host(), _want("rect"))


def test_spref_empty_input(cbg, grid):
    t = hr.from_coo(301, 257, [], [], [])
    rng = np.random.default_rng(1)
    ri, ci = rng.integers(0, 301, 77), rng.permutation(257)
    got, _, _ = _both(cbg, grid, t, ri, ci)
    assert_tiles_bits_equal(got, sr.spref(t, ri, ci))
    assert len(got["ir"]) == 0 and (got["m"], got["n"]) == (77, 257)


# ---------------------------------------------------------------------------
# 2. the sort classes' edges
# ---------------------------------------------------------------------------
def test_sort_bounds_are_the_tested_ones(cbg):
    assert cbg.spref_sort_bounds() == BOUNDS
    _, lens = sr.class_tile(BOUNDS)
    assert {b + d for b in BOUNDS for d in (-1, 0, 1)} | {0, 1, 2} <= set(lens)
    assert max(lens) > BOUNDS[-1] + 1


@pytest.mark.parametrize("order", ["reversal", "random"])
def test_sort_class_edges(cbg, grid, order):
    t, lens = sr.class_tile(BOUNDS)
    m = t["m"]
    ri = np.arange(m)[::-1].copy() if order == "reversal" else np.random.default_rng(4).permutation(m)
    got, st, st_grid = _both(cbg, grid, t, ri, None)
    assert_tiles_bits_equal(got, sr.spref(t, ri, None))
    ln = np.asarray(lens)
    for s in (st, st_grid):
        assert s["sorted_wave"] == int(np.sum((ln >= 2) & (ln <= BOUNDS[0]))) > 0, s
        assert s["sorted_lds"] == int(np.sum((ln > BOUNDS[0]) & (ln <= BOUNDS[1]))) > 0, s
        assert s["sorted_radix"] == int(np.sum(ln > BOUNDS[1])) > 0, s
        assert s["cols_monotone"] == 0 and s["ms_sort"] > 0


# ---------------------------------------------------------------------------
# 3. the reference's algorithm on the device: P * A * Q through the SUMMA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["perm", "repeats"])
def test_spref_equals_selection_products(cbg, grid, name):
    t = sr.finite_tile()
    assert np.any(np.signbit(t["val"]) & (t["val"] == 0)) and np.all(np.isfinite(t["val"]))
    ri, ci = sr.index_cases(t["m"], t["n"])[name]
    P = hr.from_coo(len(ri), t["m"], np.arange(len(ri)), ri, np.ones(len(ri)))
    Q = hr.from_coo(t["n"], len(ci), ci, np.arange(len(ci)), np.ones(len(ci)))
    A = _mat(cbg, grid, t)
    PA = cbg.Mult_AnXBn_DoubleBuff(_mat(cbg, grid, P), A)
    PAQ = cbg.Mult_AnXBn_DoubleBuff(PA, _mat(cbg, grid, Q))
    got = A.SubsRef(ri, ci)
    assert_tiles_bits_equal(got.tile.to_host(), PAQ.tile.to_host())  # every entry one product 1.0 * a
    assert_tiles_bits_equal(got.tile.to_host(), sr.spref(t, ri, ci))


# ---------------------------------------------------------------------------
# 4. the reference's own results
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.GOLDEN_CASES)
def test_spref_golden(cbg, grid, case):
    z = np.load(os.path.join(HERE, "golden", f"spref_{case}.npz"), allow_pickle=False)
    t = hr.from_coo(int(z["m"]), int(z["n"]), z["in_row"], z["in_col"], z["in_val"])
    got, _, _ = _both(cbg, grid, t, z["ri"], z["ci"])
    want = hr.from_coo(len(z["ri"]), len(z["ci"]), z["out_row"], z["out_col"], z["out_val"])
    assert_tiles_bits_equal(got, want)


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------
def test_spref_errors(cbg, grid):
    t, _ = _main()
    m, n = t["m"], t["n"]
    T = cbg.Tile.from_dict(t)
    A = _mat(cbg, grid, t)
    before = _dig(T)
    for ri, ci in (([-1], None), ([m], None), (None, [n]), (None, [-1]), ([0, m - 1, m], [0])):
        for call in (T.spref, A.SubsRef):
            with pytest.raises(cbg.CbgError) as e:
                call(ri, ci)
            assert e.value.code == cbg.INVALIDPARAMS
    L = cbg.lib()
    import ctypes
    idx = np.zeros(4, np.int64)
    out = cbg.CTile()
    assert L.cbg_tile_spref(ctypes.byref(T.c), idx.ctypes.data, -1, None, 0, ctypes.byref(out)) == cbg.INVALIDPARAMS
    assert L.cbg_grid_spref(grid.h, ctypes.byref(A.tile.c), m, n, None, 0, idx.ctypes.data, -2,
                            ctypes.byref(out)) == cbg.INVALIDPARAMS
    assert L.cbg_grid_spref(grid.h, ctypes.byref(A.tile.c), m + 1, n, None, 0, None, 0,
                            ctypes.byref(out)) == cbg.INVALIDPARAMS
    assert _dig(T) == before and _dig(A.tile) == before


# ---------------------------------------------------------------------------
# 6. HipMCL with RandPermute
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain(case, ps):
    return hr.hipmcl(hr.CASES[case](), *ps)


def _final_invariants(cbg, F, n_work):
    f = F.tile.to_host()
    assert F.tile.digest()["unsorted"] == 0 and (f["m"], f["n"]) == (n_work, n_work) and len(f["jc"]) == n_work
    lens = np.diff(f["cp"])
    sums = np.array([np.sum(f["val"][f["cp"][p]:f["cp"][p + 1]]) for p in range(len(lens))])
    assert np.all(np.abs(sums - 1.0) <= 4 * np.finfo(np.float64).eps * lens)


def _run(cbg, grid, t, ps, **prep):
    infl, h, S, R, q = ps
    seen = []
    A = _mat(cbg, grid, t)
    labels, its, F, work = cbg.HipMCL(A, inflation=infl, prunelimit=h, select=S, recover_num=R, recover_pct=q,
                                      on_iteration=lambda *a: seen.append(a), keep_final=True, return_work_ids=True,
                                      **prep)
    assert_tiles_bits_equal(A.tile.to_host(), t)  # the input is left as it was
    return labels, its, F, work, [a[1] for a in seen]


def _chaos_close(got, want, what):
    assert len(got) == len(want)
    rel = [abs(a - w) / max(w, hr.EPS) for a, w in zip(got, want)]
    print("chaos against the restatement, %s: largest relative difference %.3g" % (what, max(rel)))
    assert max(rel) <= CHAOS_RTOL, rel


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("ps", hr.PARAM_SETS, ids=["i2_select", "i1.7_threshold"])
@pytest.mark.parametrize("case", sorted(hr.CASES))
def test_hipmcl_randpermute(cbg, grid, case, ps, seed):
    t = hr.CASES[case]()
    wlab, wit, _, _ = _plain(case, ps)
    plab, pit, pchaos, pids = sr.hipmcl_prepared(t, ps, randpermute=True, seed=seed)
    assert pit == wit == (12 if ps[0] == 2.0 else 14) and np.array_equal(plab, wlab)  # the restatement itself
    labels, its, F, work, chaos = _run(cbg, grid, t, ps, randpermute=True, perm_seed=seed)
    np.testing.assert_array_equal(labels, wlab)  # the original numbering
    assert its == wit
    np.testing.assert_array_equal(work, sr.rand_perm(t["n"], seed))
    np.testing.assert_array_equal(work, pids)
    _final_invariants(cbg, F, t["n"])
    _chaos_close(chaos, pchaos, f"{case} {ps} seed {seed}")
    # the converged matrix is in the working numbering: its components, mapped back, are the labels
    back = np.empty(t["n"], np.int64)
    back[work] = cbg.Interpret(F)
    np.testing.assert_array_equal(hr.canonical(back), labels)
    st = cbg.spref_stats()
    assert st["entries_in"] == st["entries_out"] == len(t["ir"]) and st["cols_monotone"] == 0


# ---------------------------------------------------------------------------
# 7. HipMCL with RemoveIsolated
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ps", hr.PARAM_SETS, ids=["i2_select", "i1.7_threshold"])
@pytest.mark.parametrize("case", sorted(hr.CASES))
def test_hipmcl_remove_isolated(cbg, grid, case, ps):
    base = hr.CASES[case]()
    n = base["n"]
    at = sr.pad_positions(n)
    t = sr.pad_isolated(base, at)
    wlab, wit, wchaos, wids = sr.hipmcl_prepared(t, ps, remove_isolated=True)
    ulab, uit, _, _ = hr.hipmcl(t, *ps)  # without removal
    labels, its, F, work, chaos = _run(cbg, grid, t, ps, remove_isolated=True)
    np.testing.assert_array_equal(labels, wlab)
    assert its == wit
    np.testing.assert_array_equal(work, sr.nonisolated(t))
    assert len(work) == int(np.sum(hr.reduce_cols(t, "sum") > 0)) and not set(at) & set(work.tolist())
    for v in at:  # the five are singletons
        assert np.sum(labels == labels[v]) == 1
    _final_invariants(cbg, F, len(work))
    _chaos_close(chaos, wchaos, f"{case} {ps} RemoveIsolated")
    st = cbg.spref_stats()
    assert st["cols_monotone"] > 0 and st["sorted_wave"] + st["sorted_lds"] + st["sorted_radix"] == 0
    if case == "planted":  # no vertex with in-edges only: the run without removal, two isolated vertices of its own
        np.testing.assert_array_equal(labels, ulab)
        assert its == uit and len(work) == n - 2
    else:  # hub: 76 empty columns, among them vertices with in-edges only (a nonempty row), which leave with their rows
        rows = np.zeros(t["n"], bool)
        rows[t["ir"]] = True
        gone = np.setdiff1d(np.arange(t["n"]), work)
        assert len(gone) == 5 + 76 and int(np.sum(rows[gone])) > 0 and not np.array_equal(labels, ulab)
        for v in gone:
            assert np.sum(labels == labels[v]) == 1


def test_hipmcl_in_edges_only_vertex(cbg, grid):
    """planted with vertex 30's column emptied: it keeps its row (in-edges only), is removed with
    it, and the labels are the restatement's on spref(t, nonisov, nonisov) with 30 a singleton"""
    p = hr.planted()
    col = hr.cols_of(p)
    keep = col != 30
    t = hr.from_coo(p["m"], p["n"], p["ir"][keep], col[keep], p["val"][keep])
    assert np.any(t["ir"] == 30) and 30 not in t["jc"]
    ps = hr.PARAM_SETS[0]
    ids = sr.nonisolated(t)
    assert 30 not in ids
    wl, wit, _, _ = hr.hipmcl(sr.spref(t, ids, ids), *ps)
    full = np.full(t["n"], -1, np.int64)
    full[ids] = wl
    gone = np.flatnonzero(full < 0)
    full[gone] = wl.max() + 1 + np.arange(len(gone))
    labels, its, F, work, _ = _run(cbg, grid, t, ps, remove_isolated=True)
    np.testing.assert_array_equal(labels, hr.canonical(full))
    assert its == wit and np.sum(labels == labels[30]) == 1
    assert not np.array_equal(labels, hr.hipmcl(t, *ps)[0])  # without removal 30 joins its group


def test_hipmcl_both_steps(cbg, grid):
    base = hr.planted()
    t = sr.pad_isolated(base, sr.pad_positions(base["n"]))
    ps = hr.PARAM_SETS[0]
    wlab, wit, wchaos, wids = sr.hipmcl_prepared(t, ps, remove_isolated=True, randpermute=True, seed=3)
    labels, its, F, work, chaos = _run(cbg, grid, t, ps, remove_isolated=True, randpermute=True, perm_seed=3)
    np.testing.assert_array_equal(labels, wlab)
    np.testing.assert_array_equal(labels, hr.hipmcl(t, *ps)[0])
    nonisov = sr.nonisolated(t)
    np.testing.assert_array_equal(work, nonisov[sr.rand_perm(len(nonisov), 3)])
    assert its == wit
    _final_invariants(cbg, F, len(nonisov))
    _chaos_close(chaos, wchaos, "planted both steps")


def test_prepared_without_flags_is_hipmcl(cbg, grid):
    import ctypes
    t = hr.planted()
    A = _mat(cbg, grid, t)
    infl, h, S, R, q = hr.PARAM_SETS[0]
    p = cbg.CHipMclParams(infl, cbg.CMclParams(h, S, R, q), 1, 0, 0, -1, 0, 0.0, 0)
    lab, work = np.zeros(t["n"], np.int64), np.zeros(t["n"], np.int64)
    nc, its, nw = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    for prep in (None, ctypes.byref(cbg.CHipMclPrep(0, 0, 9))):
        rc = cbg.lib().cbg_grid_hipmcl_prepared(grid.h, ctypes.byref(A.tile.c), t["n"], ctypes.byref(p), prep,
                                                cbg.HIPMCL_ITER_FN(), None, None, lab.ctypes.data, ctypes.byref(nc),
                                                ctypes.byref(its), work.ctypes.data, ctypes.byref(nw))
        assert rc == 0 and nw.value == t["n"] and np.array_equal(work, np.arange(t["n"]))
        np.testing.assert_array_equal(lab, _plain("planted", hr.PARAM_SETS[0])[0])


def test_remove_isolated_and_rand_permute_mirrors(cbg, grid):
    base = hr.hub()
    t = sr.pad_isolated(base, sr.pad_positions(base["n"]))
    A = _mat(cbg, grid, t)
    B, ids = cbg.RemoveIsolated(A)
    np.testing.assert_array_equal(ids, sr.nonisolated(t))
    assert_tiles_bits_equal(B.tile.to_host(), sr.spref(t, ids, ids))
    C, p = cbg.RandPermute(B, 2)
    np.testing.assert_array_equal(p, sr.rand_perm(len(ids), 2))
    assert_tiles_bits_equal(C.tile.to_host(), sr.spref(sr.spref(t, ids, ids), p, p))
    assert A.LoadImbalance() == B.LoadImbalance() == 1.0
    with pytest.raises(cbg.CbgError) as e:
        cbg.RandPermute(_mat(cbg, grid, sr.main_tile()))
    assert e.value.code == cbg.DIMMISMATCH


# ---------------------------------------------------------------------------
# 8. tools/hipmcl_check with the two steps
# ---------------------------------------------------------------------------
def test_hipmcl_check_driver_prepared(cbg, grid, tmp_path):
    exe = os.path.join(REPO, "tools", "hipmcl_check")
    if not os.path.exists(exe):
        pytest.fail("tools/hipmcl_check is not built (make -C combblas-spmm-test_amd drivers)")
    base = hr.planted()
    t = sr.pad_isolated(base, sr.pad_positions(base["n"]))
    ps = hr.PARAM_SETS[0]
    labels, its, _, work, _ = _run(cbg, grid, t, ps, remove_isolated=True, randpermute=True, perm_seed=7)
    mtx = str(tmp_path / "a.mtx")
    cbg.write_mm(mtx, t)
    run = subprocess.run([exe, mtx] + [repr(x) if isinstance(x, float) else str(x) for x in ps] +
                         ["remove_isolated", "randpermute", "7"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "HIPMCLCHECK OK" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"iterations {its}\n" in run.stdout, (its, run.stdout[-1500:])
    assert f"clusters {labels.max() + 1} labels {_fnv1a_labels(labels)}" in run.stdout, run.stdout[-1500:]
    assert f"n_work {len(work)}" in run.stdout


# ---------------------------------------------------------------------------
# several ranks on one GPU
# ---------------------------------------------------------------------------
def _launch(nproc, args, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(HERE, "spref_worker.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = r.stdout + r.stderr
    errs = [ln for ln in out.splitlines() if "CbgError" in ln or "[cbg]" in ln or "AssertionError" in ln]
    return r.returncode, "\n".join(errs[:16]) + "\n" + out


@pytest.mark.parametrize("grid_shape", [(2, 1), (1, 2), (2, 2)])
def test_spref_multirank_host_transport(grid_shape):
    """every rank's tile of the distributed result has the bits of its block of the 1 x 1 result
    (tests/spref_worker.py lists the cases); HipMCL with both steps gives the 1 x 1 labels;
    LoadImbalance before and after RandPermute"""
    rc, out = _launch(grid_shape[0] * grid_shape[1], ["gpu", str(grid_shape[0]), str(grid_shape[1])])
    assert rc == 0 and out.count("SPREFOK") == grid_shape[0] * grid_shape[1], out[:1500] + out[-3000:]


def test_spref_multirank_rccl():
    rc, out = _launch(2, ["rccl", "2", "1"])
    assert rc == 0 and out.count("SPREFOK") == 2 and "transport rccl" in out, out[:1500] + out[-3000:]
