"""cbg_grid_bfs, cbg_tile_spmspv_max and cbg_tile_pull_max (csrc/cbg_bfs.hip, the loop in
csrc/cbg_grid_algos.cpp) against the fixtures of tests/golden/make_bfs_golden.py (the reference's own
top-down loop) and the restatement tests/bfs_ref.py.  max is exact and order-free, so everything is
compared by bits: parents, levels, the steps the callback sees, the direction string, the counts."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bfs_ref
from bfs_worker import CASES, load_case
from test_gpu_hipmcl import _self_grid
from test_multiprocess import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
hr = bfs_ref.hr


@pytest.fixture
def grid(cbg):
    g = _self_grid(cbg)
    yield g
    g.destroy()


@functools.lru_cache(maxsize=None)
def _want(name, root, direction, up=None, down=None):
    return bfs_ref.bfs(load_case(name)[1], root, direction, up, down)


def _run(cbg, A, root, direction="auto", **kw):
    seen = []
    parents, levels = cbg.BFS(A, root, direction, on_level=lambda *s: seen.append(s), **kw)
    return parents, levels, seen, cbg.bfs_stats()


@pytest.mark.parametrize("name", CASES)
def test_bfs_fixture(cbg, grid, name):
    z, a = load_case(name)
    C = cbg.bfs_bounds()[0]
    A = cbg.SpParMat.from_global(grid, a)
    before = A.tile.digest()
    for k, root in enumerate(z["roots"].tolist()):
        for direction in ("auto", "topdown", "bottomup"):
            want = _want(name, root, direction)
            parents, levels, seen, st = _run(cbg, A, root, direction)
            assert np.array_equal(parents, z["parents"][k]), (root, direction)
            assert np.array_equal(levels, want["levels"]) and np.array_equal(levels, z["levels"][k]), (root, direction)
            assert seen == want["steps"], (root, direction)
            assert "".join(s[1] for s in seen) == (str(z["traces"][k]) if direction == "auto" else want["trace"])
            ws = dict(want["stats"])
            ws["push_units"] = sum(bfs_ref.units_of(a, f, C) for f, s in zip(want["fronts"], want["steps"]) if s[1] == "d")
            assert {s: st[s] for s in ws} == ws, (root, direction, st, ws)
            assert st["ms_total"] > 0
    after = A.tile.digest()
    assert (after["hs"], after["hv"], after["nnz"]) == (before["hs"], before["hv"], before["nnz"])


# ---------------------------------------------------------------------------
# push, one tile
# ---------------------------------------------------------------------------
def _tile(cbg, m, n, r, c):
    t = hr.from_coo(m, n, r, c, np.zeros(len(r)))  # explicit zeros: every stored entry is `true`
    return t, cbg.Tile.from_dict(t)


def test_push_column_lengths_around_the_chunk(cbg):
    C = cbg.bfs_bounds()[0]
    m, n = 2 * C + 7, 12
    cols = {0: [m - 1], 1: range(0, C - 1), 3: range(0, C), 4: range(5, C + 6), 7: range(0, 2 * C + 1), 10: [2, C, m - 1],
            11: range(C - 3, C + 3)}  # 2, 5, 6, 8, 9 are not in jc
    assert [len(cols[j]) for j in (1, 3, 4, 7)] == [C - 1, C, C + 1, 2 * C + 1]
    r = np.concatenate([np.array(list(v)) for v in cols.values()])
    c = np.concatenate([np.full(len(v), j) for j, v in cols.items()])
    t, T = _tile(cbg, m, n, r, c)
    for xind in ([1, 3, 4, 7, 9], [1, 3, 4, 7], [], list(range(n)), [9], [0, 10, 11], [7]):
        yi, yv = cbg.SpMSpV(T, xind)
        wi, wv = bfs_ref.spmspv_max(t, xind)
        assert np.array_equal(yi, wi) and np.array_equal(yv, wv), xind
        assert cbg.bfs_stats()["push_units"] == bfs_ref.units_of(t, xind, C), xind
    # values out of order against the ids: the largest value wins, not the largest id
    xind = [1, 3, 4, 7, 9, 10]
    xval = [50, -7, 2 ** 40, 3, 99, -2 ** 40]
    yi, yv = cbg.SpMSpV(T, xind, xval)
    wi, wv = bfs_ref.spmspv_max(t, xind, xval)
    assert np.array_equal(yi, wi) and np.array_equal(yv, wv)
    got = dict(zip(yi.tolist(), yv.tolist()))
    assert got[0] == 50 and got[5] == 2 ** 40  # row 0: columns 1, 3, 7; row 5: column 4 as well
    assert got[m - 1] == -2 ** 40              # column 10 alone reaches the last row: a negative value is a value
    # the pull gives the same product
    yi, yv = cbg.SpMSpV(T, [1, 3, 4, 7, 9])
    pi, pv, _ = T.transpose().pull_max([1, 3, 4, 7, 9])
    assert np.array_equal(yi, pi) and np.array_equal(yv, pv)


@pytest.mark.parametrize("m", [63, 64, 65])
def test_push_row_counts_around_a_wave(cbg, m):
    rng = np.random.default_rng(m)
    n = 70
    keep = rng.random((m, n)) < 0.3
    keep[m - 1, n - 1] = keep[0, 0] = True
    r, c = np.nonzero(keep)
    t, T = _tile(cbg, m, n, r, c)
    for xind in (np.arange(n), np.sort(rng.choice(n, 11, replace=False)), [n - 1], []):
        yi, yv = cbg.SpMSpV(T, xind)
        wi, wv = bfs_ref.spmspv_max(t, xind)
        assert np.array_equal(yi, wi) and np.array_equal(yv, wv)
        pi, pv, read = T.transpose().pull_max(xind)
        assert np.array_equal(pi, wi) and np.array_equal(pv, wv) and read == bfs_ref.pull_max(t, xind)[2]


# ---------------------------------------------------------------------------
# pull, one tile
# ---------------------------------------------------------------------------
def test_pull_row_lengths_around_the_class_bound(cbg):
    S = cbg.bfs_bounds()[1]
    rng = np.random.default_rng(S)
    n = max(4 * S, 130)
    lens = [S - 1, S, S + 1, 0, 1, S + 1, S, 2 * S + 3, 64, 65, 63]
    r, c = [], []
    for i, ln in enumerate(lens):
        cols = np.sort(rng.choice(n, ln, replace=False))
        r += [i] * ln
        c += cols.tolist()
    t, T = _tile(cbg, len(lens), n, r, c)
    At = T.transpose()
    for trial in range(6):
        xind = np.sort(rng.choice(n, [0, 1, 3, S, n // 2, n][trial], replace=False))
        skip = None if trial % 2 == 0 else (rng.random(len(lens)) < 0.4).astype(np.uint8)
        pi, pv, read = At.pull_max(xind, skip)
        wi, wv, wread = bfs_ref.pull_max(t, xind, skip)
        assert np.array_equal(pi, wi) and np.array_equal(pv, wv) and read == wread, trial
        if skip is None:
            yi, yv = cbg.SpMSpV(T, xind)
            assert np.array_equal(pi, yi) and np.array_equal(pv, yv)
        else:
            assert not np.any(skip[pi])
    everything = np.ones(len(lens), np.uint8)
    pi, pv, read = At.pull_max(np.arange(n), everything)
    assert len(pi) == 0 and read == 0


def test_pull_wave_row_hit_positions(cbg):
    """a row of 130 entries (three steps of a wave: 64, 64, 2) with the only frontier hit at the last
    entry, at 63, 64, 65 from the end, at the first entry, or nowhere"""
    S = cbg.bfs_bounds()[1]
    assert 130 > S
    n = 300
    cols = np.arange(7, 7 + 2 * 130, 2)  # 130 ascending columns
    other = np.array([0, 5, 298])        # a short row beside it
    r = np.concatenate([np.full(130, 1), np.full(3, 2)])
    t, T = _tile(cbg, 4, n, r, np.concatenate([cols, other]))
    At = T.transpose()
    for from_end in (0, 63, 64, 65, 129, None):
        xind = [6] if from_end is None else [int(cols[129 - from_end])]  # column 6 is stored nowhere
        pi, pv, read = At.pull_max(xind)
        wi, wv, wread = bfs_ref.pull_max(t, xind)
        assert np.array_equal(pi, wi) and np.array_equal(pv, wv) and read == wread, from_end
        assert read == (130 if from_end is None else from_end + 1) + 3
    # two hits in one step, and hits in different steps: the largest column wins
    for xind in ([int(cols[10]), int(cols[100]), int(cols[120])], [int(cols[0]), int(cols[64])], [5, int(cols[1])]):
        pi, pv, read = At.pull_max(xind)
        wi, wv, wread = bfs_ref.pull_max(t, xind)
        assert np.array_equal(pi, wi) and np.array_equal(pv, wv) and read == wread, xind


def test_pull_equals_push_on_a_random_tile(cbg):
    rng = np.random.default_rng(300200)
    m, n = 300, 200
    keep = rng.random((m, n)) < 0.08
    keep[:, 17] = True   # a column every row holds
    keep[33, :] = True   # a row of 200 entries: the wave class
    keep[34, :] = False  # an empty row
    r, c = np.nonzero(keep)
    t, T = _tile(cbg, m, n, r, c)
    At = T.transpose()
    for k in (0, 1, 5, 40, 200):
        xind = np.sort(rng.choice(n, k, replace=False))
        yi, yv = cbg.SpMSpV(T, xind)
        pi, pv, read = At.pull_max(xind)
        wi, wv, wread = bfs_ref.pull_max(t, xind)
        assert np.array_equal(yi, pi) and np.array_equal(yv, pv)
        assert np.array_equal(pi, wi) and np.array_equal(pv, wv) and read == wread


# ---------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------
def test_tile_calls_refuse_bad_vectors(cbg):
    t, T = _tile(cbg, 5, 6, [0, 1, 4], [0, 3, 5])
    At = T.transpose()
    for bad in ([3, 1], [1, 1], [6], [-1], [0, 7]):
        with pytest.raises(cbg.CbgError) as e:
            cbg.SpMSpV(T, bad)
        assert e.value.code == cbg.INVALIDPARAMS
        with pytest.raises(cbg.CbgError) as e:
            At.pull_max(bad)
        assert e.value.code == cbg.INVALIDPARAMS
    L = cbg.lib()
    x = np.array([0, 3], np.int64)
    yi, yv = np.full(5, 77, np.int64), np.full(5, 77, np.int64)
    ny = ctypes.c_int64(77)
    tc, ac = ctypes.byref(T.c), ctypes.byref(At.c)
    assert L.cbg_tile_spmspv_max(tc, x.ctypes.data, None, -1, yi.ctypes.data, yv.ctypes.data, ctypes.byref(ny)) == cbg.INVALIDPARAMS
    assert L.cbg_tile_spmspv_max(tc, x.ctypes.data, None, 2, None, yv.ctypes.data, ctypes.byref(ny)) == cbg.INVALIDPARAMS
    assert L.cbg_tile_spmspv_max(tc, x.ctypes.data, None, 2, yi.ctypes.data, yv.ctypes.data, None) == cbg.INVALIDPARAMS
    assert L.cbg_tile_pull_max(ac, x.ctypes.data, -2, None, yi.ctypes.data, yv.ctypes.data, ctypes.byref(ny), None) == cbg.INVALIDPARAMS
    assert L.cbg_tile_pull_max(ac, x.ctypes.data, 2, None, yi.ctypes.data, None, ctypes.byref(ny), None) == cbg.INVALIDPARAMS
    assert L.cbg_tile_pull_max(ac, x.ctypes.data, 2, None, yi.ctypes.data, yv.ctypes.data, None, None) == cbg.INVALIDPARAMS
    assert ny.value == 77 and np.all(yi == 77) and np.all(yv == 77)  # nothing was written
    assert L.cbg_tile_pull_max(ac, x.ctypes.data, 2, None, yi.ctypes.data, yv.ctypes.data, ctypes.byref(ny), None) == 0
    assert ny.value == 2 and yi[:2].tolist() == [0, 1] and yv[:2].tolist() == [0, 3]


def test_bfs_refusals(cbg, grid):
    z, a = load_case("directed")
    n = a["n"]
    A = cbg.SpParMat.from_global(grid, a)
    for bad in (-1, n, n + 5):
        with pytest.raises(cbg.CbgError) as e:
            cbg.BFS(A, bad)
        assert e.value.code == cbg.INVALIDPARAMS
    with pytest.raises(cbg.CbgError) as e:
        cbg.BFS(A, 0, direction=3)
    assert e.value.code == cbg.INVALIDPARAMS
    L = cbg.lib()
    parents = np.full(n + 1, 77, np.int64)
    prm = cbg.CBfsParams(7, -1, -1, None)
    none = cbg.BFS_LEVEL_FN()
    assert L.cbg_grid_bfs(A.grid.h, ctypes.byref(A.tile.c), n, 3, ctypes.byref(prm), none, None, parents.ctypes.data, None) \
        == cbg.INVALIDPARAMS
    prm = cbg.CBfsParams(0, -1, -1, None)
    assert L.cbg_grid_bfs(A.grid.h, ctypes.byref(A.tile.c), n, 3, ctypes.byref(prm), none, None, None, None) == cbg.INVALIDPARAMS
    assert L.cbg_grid_bfs(A.grid.h, ctypes.byref(A.tile.c), n, 3, None, none, None, parents.ctypes.data, None) == cbg.INVALIDPARAMS
    # gn that the tile does not fit; a transpose of another shape
    assert L.cbg_grid_bfs(A.grid.h, ctypes.byref(A.tile.c), n + 1, 3, ctypes.byref(prm), none, None, parents.ctypes.data, None) \
        == cbg.DIMMISMATCH
    _, other = _tile(cbg, n, n + 1, [0], [0])
    with pytest.raises(cbg.CbgError) as e:
        cbg.BFS(A, 3, At=other)
    assert e.value.code == cbg.DIMMISMATCH
    assert np.all(parents == 77)  # nothing was written
    # levels may be left out
    assert L.cbg_grid_bfs(A.grid.h, ctypes.byref(A.tile.c), n, 3, ctypes.byref(prm), none, None, parents.ctypes.data, None) == 0
    assert np.array_equal(parents[:n], z["parents"][4]) and parents[n] == 77


def test_transpose_handed_over_or_left_out(cbg, grid):
    z, a = load_case("coretail")
    A = cbg.SpParMat.from_global(grid, a)
    At = A.tile.transpose()
    before = At.digest()
    for k, root in enumerate(z["roots"].tolist()):
        for direction in ("auto", "bottomup"):
            p0, l0, s0, st0 = _run(cbg, A, root, direction)
            p1, l1, s1, st1 = _run(cbg, A, root, direction, At=At)
            assert p0.tobytes() == p1.tobytes() == z["parents"][k].tobytes() and l0.tobytes() == l1.tobytes()
            assert s0 == s1 and {x: st0[x] for x in st0 if not x.startswith("ms")} == {x: st1[x] for x in st1 if not x.startswith("ms")}
    assert At.digest() == before


def test_cutoff_overrides_change_only_the_trace(cbg, grid):
    z, a = load_case("rmat")
    A = cbg.SpParMat.from_global(grid, a)
    base = _run(cbg, A, 0)
    assert "".join(s[1] for s in base[2]) == "duuu"
    for up, down in ((0, 10 ** 6), (10 ** 9, None), (0, 0), (None, 10 ** 6)):
        want = _want("rmat", 0, "auto", up, down)
        got = _run(cbg, A, 0, up_cutoff=up, down_cutoff=down)
        assert got[2] == want["steps"], (up, down)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    assert "ud" in _want("rmat", 0, "auto", 0, 10 ** 6)["trace"]          # forced back to push
    assert set(_want("rmat", 0, "auto", 10 ** 9, None)["trace"]) == {"d"}  # never pulls
    assert _want("rmat", 0, "auto", 0, 0)["trace"][0] == "u"               # pulls from the first step


def test_on_level_exception_is_raised_after_the_call(cbg, grid):
    z, a = load_case("path")
    A = cbg.SpParMat.from_global(grid, a)
    calls = []

    def boom(level, direction, frontier, pred):
        calls.append(level)
        raise ZeroDivisionError("from on_level")

    with pytest.raises(ZeroDivisionError):
        cbg.BFS(A, int(z["roots"][1]), on_level=boom)
    assert calls == list(range(1, 67))  # the collective ran to its end: depth 65, one step more


def test_bfs_check_driver(cbg, tmp_path):
    """tools/bfs_check (the C++ mirror header, TopDownBFS's `Input <file>` command line) on coretail"""
    exe = os.path.join(os.path.dirname(HERE), "tools", "bfs_check")
    if not os.path.exists(exe):
        pytest.fail("tools/bfs_check is not built (make -C combblas-spmm-test_amd drivers)")
    z, a = load_case("coretail")
    cbg.write_mm(str(tmp_path / "coretail.mtx"), a)
    run = subprocess.run([exe, "Input", str(tmp_path / "coretail.mtx")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "BFSCHECK OK" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    # its first root is the first vertex of nonzero degree, 0: depth 40, trace as the fixture's
    reached = int((z["parents"][0] >= 0).sum())
    assert f"root 0 levels 40 reached {reached} trace {z['traces'][0]}" in run.stdout, run.stdout[-1500:]


# ---------------------------------------------------------------------------
# several ranks
# ---------------------------------------------------------------------------
def _launch(nproc, args, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(HERE, "bfs_worker.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = r.stdout + r.stderr
    errs = [ln for ln in out.splitlines() if "CbgError" in ln or "[cbg]" in ln or "AssertionError" in ln]
    return r.returncode, "\n".join(errs[:16]) + "\n" + out


@pytest.mark.parametrize("grid_shape", [(2, 1), (1, 2), (2, 2)])
def test_bfs_multirank_host_transport(grid_shape):
    rc, out = _launch(grid_shape[0] * grid_shape[1], ["gpu", str(grid_shape[0]), str(grid_shape[1])])
    assert rc == 0 and out.count("BFSOK") == grid_shape[0] * grid_shape[1], out[:1500] + out[-3000:]


def test_bfs_multirank_rccl():
    rc, out = _launch(2, ["rccl", "2", "1"])
    assert rc == 0 and out.count("BFSOK") == 2 and "transport rccl" in out, out[:1500] + out[-3000:]
