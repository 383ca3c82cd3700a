"""y = A x on PlusTimes and MinPlus over a dense and a sparse vector (cbg_tile_spmv, cbg_tile_spmspv,
cbg_grid_spmv, cbg_grid_spmspv).  Every comparison is against tests/spmv_ref.py by bits unless it says
otherwise; the fixtures under tests/golden/spmv_*.npz hold the reference's own outputs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import bfs_ref
import colsum_ref as cr
import hipmcl_ref as hr
import spmv_ref as sv
from spmv_worker import CASES, SEMIRINGS, SPARSE, load_case
from test_gpu_hipmcl import _self_grid
from test_multiprocess import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DBL_MAX = sv.DBL_MAX


def same_bits(a, b):
    return np.array_equal(sv.bits(a), sv.bits(b))


def assert_sparse(got, want, what=None):
    assert np.array_equal(got[0], want[0]), what
    assert same_bits(got[1], want[1]), what


# ---------------------------------------------------------------------------
# the fixtures: the reference's own results
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("s,sr", SEMIRINGS)
def test_fixtures_on_the_1x1_grid(cbg, name, s, sr):
    z, ts = load_case(name)
    t, x = ts[s], z["x_" + s]
    exact = name == "dyadic" or sr == sv.MIN_PLUS
    g = _self_grid(cbg)
    A = cbg.SpParMat(cbg.Tile.from_dict(t), g, t["m"], t["n"])
    want = sv.spmv(t, x, sr)
    for y in (cbg.SpMV(A, x, sr), A.tile.spmv(x, sr), cbg.SpMV(A, x, sr, At=A.tile.transpose())):
        assert same_bits(y, want)
        for ref, pc in ((z["y_" + s], 1), (z["y4_" + s], 2)):
            if exact:
                assert same_bits(y, ref)
            else:  # two orderings of the same rounded products: every row
                assert np.all(np.abs(y - ref) <= sv.bound(t, x, pc=pc))
    for k in SPARSE:
        ids = z["xs_" + k]
        want = sv.spmspv(t, ids, x[ids], sr)
        for got in (cbg.SpMV_sparse(A, ids, x[ids], sr), A.tile.spmspv(ids, x[ids], sr)):
            assert_sparse(got, want, (name, s, k))
            for pre, pc in (("ys", 1), ("ys4", 2)):
                ri, rv = z[f"{pre}_{s}_{k}_ind"], z[f"{pre}_{s}_{k}_val"]
                assert np.array_equal(got[0], ri)
                if exact:
                    assert same_bits(got[1], rv)
                else:
                    sub = sv.restrict_cols(t, ids)
                    assert np.all(np.abs(got[1] - rv) <= sv.bound(sub, x, pc=pc)[ri])
    g.destroy()


# ---------------------------------------------------------------------------
# row lengths around every class bound
# ---------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8192, 8193, 12289)
PER_LENGTH = 3
_cache = {}


def lengths_case():
    """PER_LENGTH rows of every length of ROW_LENGTHS at n = 12 300, `wide` values, x U[-1, 1)"""
    if "lengths" not in _cache:
        rng = np.random.default_rng(12300)
        n = 12300
        lens = [ln for ln in ROW_LENGTHS for _ in range(PER_LENGTH)]
        order = rng.permutation(len(lens))
        rows, cols = [], []
        for r, k in enumerate(order):
            c = np.sort(rng.choice(n, lens[k], replace=False))
            rows.append(np.full(len(c), r))
            cols.append(c)
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        t = hr.from_coo(len(lens), n, rows, cols, cr.pattern_values(rng, "wide", len(rows)))
        _cache["lengths"] = t, rng.uniform(-1.0, 1.0, n)
    return _cache["lengths"]


def expected_classes(lens):
    lens = np.asarray(lens)
    lens = lens[lens > 0]
    long_ = lens[lens > sv.WAVE_MAX]
    return dict(rows_group=int((lens <= sv.GROUP_MAX).sum()),
                rows_wave=int(((lens > sv.GROUP_MAX) & (lens <= sv.WAVE_MAX)).sum()), rows_long=len(long_),
                chunks=int((-(-long_ // sv.WAVE_MAX)).sum()))


def test_bounds(cbg):
    assert cbg.spmv_bounds()[:2] == [sv.GROUP_MAX, sv.WAVE_MAX] and cbg.spmv_bounds()[2] >= 64


@pytest.mark.parametrize("s,sr", SEMIRINGS)
def test_row_lengths_around_every_class_bound(cbg, s, sr):
    t, x = lengths_case()
    lens = sv.row_lengths(t)
    assert sorted(set(lens.tolist())) == sorted(ROW_LENGTHS)
    A = cbg.Tile.from_dict(t)
    want = sv.spmv(t, x, sr)
    y = A.spmv(x, sr)
    assert same_bits(y, want)
    st = cbg.spmv_stats()
    exp = expected_classes(lens)
    assert {k: st[k] for k in exp} == exp and min(exp.values()) > 0
    assert exp["chunks"] == PER_LENGTH * (2 + 2 + 3 + 4)
    # the sparse product with every column: the same sums, without the fold with id
    ids = np.arange(t["n"])
    wi, wv = sv.spmspv(t, ids, x, sr)
    got = A.spmspv(ids, x, sr)
    assert_sparse(got, (wi, wv))
    assert np.array_equal(wi, np.flatnonzero(lens > 0))
    assert same_bits(np.array([sv.fold_id(sr, r) for r in got[1]]), y[wi])
    st = cbg.spmv_stats()
    C = cbg.spmv_bounds()[2]
    assert {k: st[k] for k in exp} == exp
    assert st["products"] == len(t["ir"]) and st["entries_out"] == len(wi)
    assert st["units"] == int((-(-np.diff(t["cp"]) // C)).sum())


# ---------------------------------------------------------------------------
# sparse vector shapes
# ---------------------------------------------------------------------------
def tall_case(cbg):
    """m = 800: columns of exactly C - 1, C, C + 1 and 3 C + 1 entries among random ones; every 7th column empty"""
    C = cbg.spmv_bounds()[2]
    key = ("tall", C)
    if key not in _cache:
        rng = np.random.default_rng(800)
        m, n = 3 * C + 40, 90
        special = {3: C - 1, 10: C, 11: C + 1, 40: 3 * C + 1, 89: C}
        rows, cols = [], []
        for j in range(n):
            if j % 7 == 6:
                continue
            ln = special.get(j, int(rng.integers(1, 40)))
            rows.append(np.sort(rng.choice(m, ln, replace=False)))
            cols.append(np.full(ln, j))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        _cache[key] = hr.from_coo(m, n, rows, cols, cr.pattern_values(rng, "normal", len(rows))), rng.uniform(-1, 1, n), special
    return _cache[key]


@pytest.mark.parametrize("s,sr", SEMIRINGS)
def test_sparse_vector_shapes(cbg, s, sr):
    t, x, special = tall_case(cbg)
    C = cbg.spmv_bounds()[2]
    A = cbg.Tile.from_dict(t)
    n = t["n"]
    stored = set(t["jc"].tolist())
    empty = [j for j in range(n) if j not in stored]
    assert len(empty) >= 10
    shapes = dict(none=[], one=[10], one_empty=[empty[0]], two=[3, 40], all=list(range(n)),
                  special=sorted(special), special_and_empty=sorted(list(special) + empty[:5]), only_empty=empty,
                  last=[n - 1])
    for what, ids in shapes.items():
        ids = np.array(ids, np.int64)
        got = A.spmspv(ids, x[ids], sr)
        assert_sparse(got, sv.spmspv(t, ids, x[ids], sr), (what, s))
        st = cbg.spmv_stats()
        lens = cr.column_lengths(t)[ids]
        assert st["products"] == int(lens.sum()) and st["units"] == int((-(-lens // C)).sum()), what
        assert st["entries_out"] == len(got[0])
    assert len(A.spmspv([], [], sr)[0]) == 0 and len(A.spmspv(empty, x[empty], sr)[0]) == 0


def test_one_expansion_plan_for_both_sparse_products(cbg):
    """Tile.spmspv (both semirings) and the SelectMax SpMSpV push expand x's columns through the same plan:
    one list over columns of 1, 255, 256, 257 and 513 stored entries and a column that stores nothing, and
    lists of one column, give each product's reference and the same units, sum of ceil(len / bound)"""
    C = cbg.spmv_bounds()[2]
    assert C == cbg.bfs_bounds()[0]
    rng = np.random.default_rng(513)
    m, n = 520, 9
    lens = {0: 1, 2: 255, 3: 256, 5: 257, 8: 513}  # 1, 4, 6, 7 store nothing
    rows = [np.sort(rng.choice(m, ln, replace=False)) for ln in lens.values()]
    cols = [np.full(ln, j) for j, ln in lens.items()]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    t = hr.from_coo(m, n, rows, cols, cr.pattern_values(rng, "normal", len(rows)))
    assert cr.column_lengths(t).tolist() == [lens.get(j, 0) for j in range(n)]
    A = cbg.Tile.from_dict(t)
    x = rng.uniform(-1, 1, n)
    for ids in ([0, 2, 3, 4, 5, 8], [8], [3], [4]):
        ids = np.array(ids, np.int64)
        units = sum(-(-lens.get(j, 0) // C) for j in ids.tolist())
        for s, sr in SEMIRINGS:
            assert_sparse(A.spmspv(ids, x[ids], sr), sv.spmspv(t, ids, x[ids], sr), (ids, s))
            assert cbg.spmv_stats()["units"] == units, (ids, s)
        yi, yv = cbg.SpMSpV(A, ids)
        wi, wv = bfs_ref.spmspv_max(t, ids)
        assert np.array_equal(yi, wi) and np.array_equal(yv, wv), ids
        assert cbg.bfs_stats()["push_units"] == units == cbg.spmv_stats()["units"], ids


@pytest.mark.parametrize("m", [63, 64, 65])
def test_sparse_small_heights_and_a_cancelled_sum(cbg, m):
    rng = np.random.default_rng(m)
    n = 70
    mask = rng.random((n, m)) < 0.3
    mask[:, 5] = False
    mask[[2, 9], 5] = True  # row 5: exactly the columns 2 and 9
    col, row = np.nonzero(mask)
    val = cr.pattern_values(rng, "normal", len(row))
    x = rng.uniform(-1, 1, n)
    val[(row == 5) & (col == 2)], val[(row == 5) & (col == 9)] = 3.0, -1.5
    x[2], x[9] = 0.5, 1.0  # 1.5 - 1.5
    t = hr.from_coo(m, n, row, col, val)
    A = cbg.Tile.from_dict(t)
    for sr in (sv.PLUS_TIMES, sv.MIN_PLUS):
        for ids in (np.arange(n), np.array([2, 9]), np.array([0]), np.array([n - 1]), np.arange(1, n, 3)):
            assert_sparse(A.spmspv(ids, x[ids], sr), sv.spmspv(t, ids, x[ids], sr), (m, sr, len(ids)))
        assert same_bits(A.spmv(x, sr), sv.spmv(t, x, sr))
    yi, yv = A.spmspv([2, 9], x[[2, 9]])
    k = int(np.flatnonzero(yi == 5)[0])
    assert yv[k] == 0.0 and not np.signbit(yv[k])  # a cancelled sum stays as a stored +0.0


# ---------------------------------------------------------------------------
# the transpose handed over, left out, or alone; device pointers
# ---------------------------------------------------------------------------
def _raw_spmv(cbg, A, At, sr, x, m, on_device=0, xptr=None, yptr=None):
    y = np.zeros(max(m, 1))
    rc = cbg.lib().cbg_tile_spmv(ctypes.byref(A.c) if A is not None else None, ctypes.byref(At.c) if At is not None else None,
                                 sr, xptr if on_device else x.ctypes.data, yptr if on_device else y.ctypes.data,
                                 on_device, None)
    assert rc == 0, cbg.lib().cbg_last_error()
    return y[:m]


@pytest.mark.parametrize("s,sr", SEMIRINGS)
def test_transpose_given_left_out_or_alone(cbg, s, sr):
    z, ts = load_case("rect")
    t, x = ts[s], np.ascontiguousarray(z["x_" + s])
    A = cbg.Tile.from_dict(t)
    At = A.transpose()
    want = sv.spmv(t, x, sr)
    for a, at in ((A, None), (A, At), (None, At)):
        assert same_bits(_raw_spmv(cbg, a, at, sr, x, t["m"]), want)
    assert same_bits(A.spmv(x, sr, At=At), want)


def _device_vector(cbg, v):
    """a device buffer of len(v) doubles through the tile API: the values of a one-column tile"""
    n = len(v)
    return cbg.Tile.from_host(n, 1, [0, n], [0], np.arange(n), v)


@pytest.mark.parametrize("s,sr", SEMIRINGS)
def test_device_pointers_give_the_host_call_s_bits(cbg, s, sr):
    t, x = lengths_case()
    A = cbg.Tile.from_dict(t)
    At = A.transpose()
    host = A.spmv(x, sr, At=At)
    dx, dy = _device_vector(cbg, x), _device_vector(cbg, np.full(t["m"], np.nan))
    for a, at in ((A, At), (None, At), (A, None)):
        _raw_spmv(cbg, a, at, sr, x, t["m"], 1, dx.c.val, dy.c.val)
        st = cbg.spmv_stats()  # waits for the asynchronous product
        assert same_bits(dy.to_host()["val"], host)
        assert st["rows_long"] == 12 and st["ms"] > 0
    assert same_bits(host, sv.spmv(t, x, sr))


# ---------------------------------------------------------------------------
# special values
# ---------------------------------------------------------------------------
def special_case():
    """row 0: inf and -inf products; 1: a subnormal sum; 2: DBL_MAX sentinels; 3: all -0.0; 4: empty;
    5: one entry; 6: 20 entries of -0.0 (the wave class); 7: overflow to inf"""
    n = 40
    rows = {0: ([1, 4, 9], [np.inf, 2.0, -np.inf]), 1: ([0, 3, 5, 8], [5e-324, 1.5e-323, 1e-323, 2.5e-323]),
            2: ([2, 6, 7], [DBL_MAX, 4.0, 0.25]), 3: ([1, 2, 3], [-0.0, -0.0, -0.0]), 5: ([39], [-2.5]),
            6: (list(range(10, 30)), [-0.0] * 20), 7: ([0, 1], [DBL_MAX, DBL_MAX])}
    r = np.concatenate([np.full(len(c), i) for i, (c, _) in rows.items()])
    c = np.concatenate([np.array(c) for c, _ in rows.values()])
    v = np.concatenate([np.array(v, np.float64) for _, v in rows.values()])
    x = np.ones(n)
    x[6] = DBL_MAX  # MinPlus: inf_plus in row 2
    x[7] = -3.0
    return hr.from_coo(8, n, r, c, v), x


def test_special_values(cbg):
    t, x = special_case()
    A = cbg.Tile.from_dict(t)
    ids = np.arange(t["n"])
    # PlusTimes: NaN == NaN against the restatement, everything else by bits
    y, want = A.spmv(x), sv.spmv(t, x)
    assert np.isnan(y[0]) and np.isnan(want[0]) and same_bits(y[1:], want[1:])
    assert y[1] == 5.5e-323 and y[4] == 0.0 and y[5] == -2.5 and y[7] == np.inf
    yi, yv = A.spmspv(ids, x)
    wi, wv = sv.spmspv(t, ids, x)
    assert np.array_equal(yi, wi) and np.isnan(yv[0]) and np.isnan(wv[0]) and same_bits(yv[1:], wv[1:])
    # documented: an all -0.0 row gives +0.0 in the dense result (0.0 + r) and -0.0 in the sparse one
    for row in (3, 6):
        assert y[row] == 0.0 and not np.signbit(y[row])
        k = int(np.flatnonzero(yi == row)[0])
        assert yv[k] == 0.0 and np.signbit(yv[k])
    # MinPlus without the rows of inf - inf (row 0 holds both signs of inf: a + x is still defined)
    y, want = A.spmv(x, sv.MIN_PLUS), sv.spmv(t, x, sv.MIN_PLUS)
    assert same_bits(y, want)
    assert y[2] == -2.75 and y[4] == DBL_MAX and y[7] == DBL_MAX and y[0] == -np.inf
    only = np.array([2, 6])  # row 2: inf_plus(DBL_MAX, 1) and inf_plus(4, DBL_MAX), both DBL_MAX
    yi, yv = A.spmspv(only, x[only], sv.MIN_PLUS)
    assert_sparse((yi, yv), sv.spmspv(t, only, x[only], sv.MIN_PLUS))
    assert yv[int(np.flatnonzero(yi == 2)[0])] == DBL_MAX


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def test_refusals_do_no_device_work(cbg):
    z, ts = load_case("rect")
    t, x = ts["pt"], np.ascontiguousarray(z["x_pt"])
    A = cbg.Tile.from_dict(t)
    At = A.transpose()
    g = _self_grid(cbg)
    L = cbg.lib()
    m, n = t["m"], t["n"]
    y, yi, yv, ny = np.zeros(m), np.zeros(m, np.int64), np.zeros(m), ctypes.c_int64()
    a, at = ctypes.byref(A.c), ctypes.byref(At.c)
    good, vals = np.array([1, 5, 9], np.int64), np.ones(3)

    def spv(ids, cnt=None, sr=0, out=(yi, yv, ny)):
        ids = np.array(ids, np.int64)
        return L.cbg_tile_spmspv(a, sr, ids.ctypes.data, np.ones(max(len(ids), 1)).ctypes.data, len(ids) if cnt is None else cnt,
                                 out[0].ctypes.data if out[0] is not None else None,
                                 out[1].ctypes.data if out[1] is not None else None,
                                 ctypes.byref(out[2]) if out[2] is not None else None)

    def gspv(ids, cnt=None, sr=0, gm=m, gn=n):
        ids = np.array(ids, np.int64)
        return L.cbg_grid_spmspv(g.h, a, gm, gn, sr, ids.ctypes.data, np.ones(max(len(ids), 1)).ctypes.data,
                                 len(ids) if cnt is None else cnt, yi.ctypes.data, yv.ctypes.data, ctypes.byref(ny))

    before = cbg.pool_stats()
    bad, dim = cbg.INVALIDPARAMS, cbg.DIMMISMATCH
    calls = [
        (bad, lambda: L.cbg_tile_spmv(a, at, 2, x.ctypes.data, y.ctypes.data, 0, None)),
        (bad, lambda: L.cbg_tile_spmv(a, at, -1, x.ctypes.data, y.ctypes.data, 0, None)),
        (bad, lambda: L.cbg_tile_spmv(None, None, 0, x.ctypes.data, y.ctypes.data, 0, None)),
        (bad, lambda: L.cbg_tile_spmv(a, at, 0, x.ctypes.data, None, 0, None)),
        (dim, lambda: L.cbg_tile_spmv(a, a, 0, x.ctypes.data, y.ctypes.data, 0, None)),
        (bad, lambda: spv([1, 5, 9], sr=7)),
        (bad, lambda: spv([5, 1, 9])),
        (bad, lambda: spv([1, 5, 5])),
        (bad, lambda: spv([1, 5, n])),
        (bad, lambda: spv([-1, 5])),
        (bad, lambda: spv([1, 5], cnt=-1)),
        (bad, lambda: spv([1, 5], out=(None, yv, ny))),
        (bad, lambda: spv([1, 5], out=(yi, None, ny))),
        (bad, lambda: spv([1, 5], out=(yi, yv, None))),
        (bad, lambda: L.cbg_grid_spmv(g.h, a, at, m, n, 3, x.ctypes.data, y.ctypes.data)),
        (bad, lambda: L.cbg_grid_spmv(g.h, None, None, m, n, 0, x.ctypes.data, y.ctypes.data)),
        (bad, lambda: L.cbg_grid_spmv(g.h, a, None, m, n, 0, x.ctypes.data, None)),
        (dim, lambda: L.cbg_grid_spmv(g.h, a, a, m, n, 0, x.ctypes.data, y.ctypes.data)),
        (dim, lambda: L.cbg_grid_spmv(g.h, a, at, m + 1, n, 0, x.ctypes.data, y.ctypes.data)),
        (dim, lambda: L.cbg_grid_spmv(g.h, a, None, m, n - 1, 0, x.ctypes.data, y.ctypes.data)),
        (bad, lambda: gspv([1, 5], sr=2)),
        (bad, lambda: gspv([5, 1])),
        (bad, lambda: gspv([1, n])),
        (bad, lambda: gspv([1, 5], cnt=-2)),
        (dim, lambda: gspv([1, 5], gm=m + 1)),
        (dim, lambda: gspv([1, 5], gn=n + 1)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, (k, L.cbg_last_error())
        assert cbg.pool_stats() == before, k
    with pytest.raises(cbg.CbgError) as e:
        A.spmv(x, "minplus", At=A)
    assert e.value.code == dim
    # and the good calls still run
    assert same_bits(A.spmv(x, At=At), sv.spmv(t, x))
    assert_sparse(A.spmspv(good, vals), sv.spmspv(t, good, vals))
    g.destroy()


def test_empty_tiles_answer_without_a_kernel(cbg):
    E = cbg.Tile.from_host(5, 4, [0], [], [], [])
    before = cbg.pool_stats()
    for sr, ident in ((sv.PLUS_TIMES, 0.0), (sv.MIN_PLUS, DBL_MAX)):
        assert np.array_equal(E.spmv(np.ones(4), sr), np.full(5, ident))
        yi, yv = E.spmspv([0, 2], [1.0, 2.0], sr)
        assert len(yi) == 0 and len(yv) == 0
        st = cbg.spmv_stats()
        assert st["rows_group"] + st["rows_wave"] + st["rows_long"] + st["units"] == 0
    assert cbg.pool_stats() == before


# ---------------------------------------------------------------------------
# the C++ mirror's driver
# ---------------------------------------------------------------------------
def test_cpp_multtest_driver_with_vectors():
    """tools/multtest A B C x y on the sevenvertex fixture prints the reference's success lines"""
    repo = os.path.dirname(HERE)
    exe = os.path.join(repo, "tools", "multtest")
    if not os.path.exists(exe):
        pytest.skip("tools/multtest not built (needs MPICH in /opt/conda)")
    g = os.path.join(repo, "tests", "golden")
    r = subprocess.run([exe, os.path.join(g, "sevenvertex.mtx"), os.path.join(g, "sevenvertex.mtx"),
                        os.path.join(g, "sevenvertex_C.mtx"), os.path.join(g, "sevenvertex_x.txt"),
                        os.path.join(g, "sevenvertex_y.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("Dense SpMV (fully dist) working correctly", "Sparse SpMV (fully dist) working correctly",
                 "Synchronous Multiplication working correctly", "Double buffered multiplication working correctly"):
        assert line in r.stdout, r.stdout
    assert "ERROR" not in r.stdout


# ---------------------------------------------------------------------------
# several ranks
# ---------------------------------------------------------------------------
def _launch(nproc, args, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(HERE, "spmv_worker.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = r.stdout + r.stderr
    errs = [ln for ln in out.splitlines() if "CbgError" in ln or "[cbg]" in ln or "AssertionError" in ln]
    return r.returncode, "\n".join(errs[:16]) + "\n" + out


@pytest.mark.parametrize("grid_shape", [(2, 1), (1, 2), (2, 2)])
def test_spmv_multirank_host_transport(grid_shape):
    rc, out = _launch(grid_shape[0] * grid_shape[1], ["gpu", str(grid_shape[0]), str(grid_shape[1])])
    assert rc == 0 and out.count("SPMVOK") == grid_shape[0] * grid_shape[1], out[:1500] + out[-3000:]


def test_spmv_multirank_rccl():
    rc, out = _launch(4, ["rccl", "2", "2"])
    assert rc == 0 and out.count("SPMVOK") == 4 and "transport rccl" in out, out[:1500] + out[-3000:]
