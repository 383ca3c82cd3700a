"""Markov-clustering pruning on device (csrc/cbg_prune.hip) against the NumPy
restatement (tests/mcl_ref.py, pinned to the reference by tests/test_mcl_cpu.py).
All values are exact (multiples of 2^-10 with exact column sums), so every
comparison is structure-exact and value-bit-exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import colsum_ref as cr
import mcl_ref
from helpers import assert_tiles_bits_equal, load_npz
from test_multiprocess import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
M_BIG = 32768


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def _mat(cbg, g, d):
    return cbg.SpParMat(cbg.Tile.from_dict(d), g, d["m"], d["n"])


@functools.lru_cache(maxsize=None)
def _big():
    return mcl_ref.big_case()


# ---------------------------------------------------------------------------
# k-select
# ---------------------------------------------------------------------------
def _patterns(rng, n):
    """value patterns of a column of n entries"""
    i = np.arange(n, dtype=np.uint64)
    low = (np.uint64(0x3FF0000000000000) + (i * np.uint64(37)) % np.uint64(256)).view(np.float64)  # lowest key byte only
    tops = np.array([0x00, 0x01, 0x3F, 0x40, 0x7F, 0x80, 0x81, 0xBF, 0xC0, 0xFF], np.uint64)
    high = ((tops[(i * np.uint64(7)) % np.uint64(len(tops))] << np.uint64(56)) | np.uint64(0x000123456789AB)).view(np.float64)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, -1.0, 1.0, -0.5, 0.5,
                        -1e300, 1e300])
    return {
        "random": mcl_ref.dyadic(rng, n, -0.5, 0.5),
        "equal": np.full(n, 0.375),
        "two_values": np.where(i % np.uint64(2) == 0, 0.25, 0.5),
        "low_byte": low,
        "high_byte": high,
        "special": special[rng.integers(0, len(special), n)],
    }


def test_kselect_every_class(cbg):
    """cbg_grid_kselect on a self grid: lengths at bound-1, bound, bound+1 of every
    class and 1; k = 1, len-1, len, len+1 and the middle; all-equal columns, ties over
    the k-th place, values that differ in the lowest / highest key byte only,
    negatives, subnormals, both zeros.  Every kernel class must have run."""
    bounds = cbg.mcl_kselect_bounds()
    lens = [1, 2, 65] + [b + d for b in bounds for d in (-1, 0, 1)] + [20000]
    assert max(lens) <= M_BIG
    rng = np.random.default_rng(7)
    cols = []
    for ln in lens:
        for name, v in _patterns(rng, ln).items():
            rng.shuffle(v)
            cols.append(v)
    t = mcl_ref.build_tile(rng, M_BIG, len(cols) + 40, cols)
    g = _self_grid(cbg)
    A = _mat(cbg, g, t)
    srt = [np.sort(c)[::-1] for c in cols]
    ids = t["jc"]
    empty = np.setdiff1d(np.arange(t["n"]), ids)[:3].astype(np.int32)
    ks = sorted({1, 2, 3, 33, 10000, 10 ** 7} | {ln + d for ln in lens for d in (-1, 0, 1) if ln + d >= 1}
                | {max(1, ln // 2) for ln in lens})
    ran = dict.fromkeys(cbg.MCL_KSELECT_CLASSES, 0)
    for k in ks:
        got = A.Kselect(np.concatenate([ids, empty]), k)
        for c, n in cbg.mcl_stats()["kselect"].items():
            ran[c] += n
        want = np.array([s[min(k, len(s)) - 1] + 0.0 for s in srt] + [0.0] * len(empty))
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert len(bad) == 0, (k, [(int(i), len(srt[i]) if i < len(srt) else 0, got[i], want[i]) for i in bad[:6]])
    assert all(n > 0 for n in ran.values()), ran
    # a subset in another order, and the argument checks that need a device tile
    sub = ids[::-5].copy()
    got = A.Kselect(sub, 3)
    want = np.array([srt[i][min(3, len(srt[i])) - 1] + 0.0 for i in range(len(ids))[::-5]])
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    for badcols in ([int(ids[0]), int(ids[0])], [t["n"]], [-1]):
        with pytest.raises(cbg.CbgError) as e:
            A.Kselect(badcols, 1)
        assert e.value.code == cbg.INVALIDPARAMS
    g.destroy()


# ---------------------------------------------------------------------------
# column statistics and PruneColumn
# ---------------------------------------------------------------------------
def test_col_stats_strict_and_not(cbg):
    t = _big()
    T = cbg.Tile.from_dict(t)
    thr = np.full(t["n"], mcl_ref.H)
    for p, j in enumerate(t["jc"]):  # a value of the column itself: strict and non-strict differ
        c = t["val"][t["cp"][p]:t["cp"][p + 1]]
        thr[j] = np.sort(c)[len(c) // 2]
    differ = 0
    for strict in (1, 0):
        cnt, tot = T.col_stats(thr, strict)
        wc, ws = mcl_ref.col_stats_ref(t, thr, strict)
        np.testing.assert_array_equal(cnt, wc)
        np.testing.assert_array_equal(tot, ws)  # exact sums: any order gives these bits (a zero's sign aside)
        differ += int(cnt.sum())
    s1 = T.col_stats(thr, 1)[0].sum()
    assert differ - 2 * s1 >= len(t["jc"])  # every column holds its threshold at least once
    cnt, tot = T.col_stats(mcl_ref.H, 1)  # one value for all columns
    np.testing.assert_array_equal(cnt, mcl_ref.col_stats_ref(t, np.full(t["n"], mcl_ref.H), 1)[0])


@pytest.mark.parametrize("pattern", cr.PATTERNS)
def test_col_stats_ordered_bits(cbg, pattern):
    """inexact values: counts and sums of the kept values by bits against the order-exact
    restatement (tests/colsum_ref.py); the threshold is the column's own median, so the kept
    set is a strict subset and the strict and the non-strict result differ"""
    t = cr.inexact_case(pattern)
    T = cbg.Tile.from_dict(t)
    thr = np.zeros(t["n"])
    for p, j in enumerate(t["jc"]):
        c = t["val"][t["cp"][p]:t["cp"][p + 1]]
        thr[j] = np.sort(c)[len(c) // 2]
    lens = cr.column_lengths(t)
    res = {}
    for strict in (1, 0):
        cnt, tot = T.col_stats(thr, strict)
        wc, ws = cr.col_stats_ordered(t, thr, strict)
        np.testing.assert_array_equal(cnt, wc)
        bad = np.flatnonzero(tot.view(np.uint64) != ws.view(np.uint64))
        assert len(bad) == 0, (pattern, strict, "%d columns differ; first: length %d, got %s, want %s" % (
            len(bad), lens[bad[0]], float(tot[bad[0]]).hex(), float(ws[bad[0]]).hex()))
        assert np.all(cnt[lens > 1] < lens[lens > 1])  # a strict subset is kept
        res[strict] = (cnt, tot)
    assert np.all(res[0][0][lens > 0] > res[1][0][lens > 0])
    assert np.any(res[0][1].view(np.uint64) != res[1][1].view(np.uint64))


def _prune_emptied(cbg, t):
    """the first, the last, a middle column emptied, several, none (nothing pruned at all), all"""
    T = cbg.Tile.from_dict(t)
    jc = t["jc"]
    nzc = len(jc)
    several = sorted({0, min(1, nzc - 1), nzc // 2, max(nzc - 2, 0), nzc - 1})
    for emptied in ([0], [nzc - 1], [nzc // 2], several, [], list(range(nzc))):
        thr = np.full(t["n"], mcl_ref.H if emptied else -1e300)
        thr[jc[emptied]] = 1e300
        out = T.prune_column(thr)
        want = mcl_ref.prune_columns(t, thr[jc])
        assert out.digest()["unsorted"] == 0
        assert out.nzc == len(want["jc"]) and out.nnz == len(want["ir"])
        assert_tiles_bits_equal(out.to_host(), want)
        if not emptied:
            assert_tiles_bits_equal(want, t)
    assert out.nnz == 0 and out.nzc == 0  # the all-pruned tile is the empty tile


def test_prune_column_emptied_columns(cbg):
    """on the big case, and on 1, 4, 5, 2048 and 2049 stored columns of 1, 63, 64, 65 and 130
    entries (a wave, a block of four waves and one more, the slot scan's second level; the
    64-lane ballot round of the filtered copy)"""
    import tile_ops_ref
    for k in tile_ops_ref.REBUILD_SLOTS:
        _prune_emptied(cbg, tile_ops_ref.rebuild_case(k))
    t = _big()
    T = cbg.Tile.from_dict(t)
    jc = t["jc"]
    nzc = len(jc)
    _prune_emptied(cbg, t)
    # thresholds of the columns' own values: entries equal to the threshold stay
    thr = np.zeros(t["n"])
    for p, j in enumerate(jc):
        thr[j] = np.max(t["val"][t["cp"][p]:t["cp"][p + 1]])
    out = T.prune_column(thr)
    assert_tiles_bits_equal(out.to_host(), mcl_ref.prune_columns(t, thr[jc]))
    assert out.nzc == nzc


# ---------------------------------------------------------------------------
# MCLPruneRecoverySelect on one tile
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mcl_a.npz", "mcl_b.npz", "big"])
def test_mcl_prune_against_restatement(cbg, case):
    if case == "big":
        t = _big()
    else:
        z = np.load(os.path.join(HERE, "golden", case), allow_pickle=False)
        t = dict(m=int(z["m"]), n=int(z["n"]), cp=z["cp"].astype(np.int64), jc=z["jc"].astype(np.int32),
                 ir=z["ir"].astype(np.int32), val=z["val"].astype(np.float64))
    g = _self_grid(cbg)
    A = _mat(cbg, g, t)
    for k, (h, S, R, q) in enumerate(mcl_ref.PARAM_SETS):
        took = {}
        want = mcl_ref.mcl_prune_ref(t, h, S, R, q, took)
        P = cbg.MCLPruneRecoverySelect(A, h, S, R, q)
        st = cbg.mcl_stats()
        assert P.tile.digest()["unsorted"] == 0
        assert_tiles_bits_equal(P.tile.to_host(), want)
        assert st["entries_in"] == len(t["ir"]) and st["entries_out"] == len(want["ir"]) and st["pieces"] == 1
        assert st["cols_recovered"] == len(took["recovery"])
        assert st["cols_selected"] == len(took["selection"])
        assert st["cols_recovered_after"] == len(took["recovery_after_selection"])
        if case != "big":  # the reference's own output
            np.testing.assert_array_equal(P.tile.to_host()["val"].view(np.uint64), z[f"out{k}_val"].view(np.uint64))
        elif (S, R) == (mcl_ref.S_NUM, mcl_ref.R_NUM):
            assert all(n > 0 for n in st["kselect"].values()), st
    # no pruning at all: a copy
    P = cbg.MCLPruneRecoverySelect(A, 0.0, 0, 0, 0.0)
    assert_tiles_bits_equal(P.tile.to_host(), t)
    assert A.tile.nnz == len(t["ir"])  # the input is left as it is
    g.destroy()


# ---------------------------------------------------------------------------
# end to end: the pruned phased product
# ---------------------------------------------------------------------------
E2E = (0.0625, 20, 30, 4.0)


@functools.lru_cache(maxsize=None)
def _product(scale):
    """(A with exact values, unpruned A*A on host, its restatement-pruned form)"""
    from conftest import load_cbg
    cbg = load_cbg()
    g = _self_grid(cbg)
    a = mcl_ref.dyadic_values(cbg.rmat_tile(scale, 16).to_host())
    A, B = _mat(cbg, g, a), _mat(cbg, g, a)
    C = cbg.MemEfficientSpGEMM(A, B, 1).tile.to_host()
    took = {}
    want = mcl_ref.mcl_prune_ref(C, *E2E, took)
    assert took["selection"] and took["recovery"], {k: len(v) for k, v in took.items()}
    return a, C, want, g


@pytest.mark.parametrize("scale", [10, 12])
def test_memefficient_mcl_end_to_end(cbg, scale):
    a, C, want, g = _product(scale)
    A, B = _mat(cbg, g, a), _mat(cbg, g, a)
    digests = set()
    for exec_mode in (cbg.EXEC_PANEL, cbg.EXEC_STAGED):
        for phases in (1, 3, cbg.PHASES_AUTO):
            P = cbg.MemEfficientSpGEMM_MCL(A, B, phases, *E2E, exec_mode=exec_mode)
            st = cbg.mcl_stats()
            assert st["entries_in"] == len(C["ir"]) and st["entries_out"] == len(want["ir"])
            assert st["pieces"] >= (3 if phases == 3 else 1)
            d = P.tile.digest()
            assert d["unsorted"] == 0
            digests.add((d["nnz"], d["nzc"], d["hs"], d["hv"]))
            assert_tiles_bits_equal(P.tile.to_host(), want)
    assert len(digests) == 1  # identical across phases and exec modes
    # streaming: pruned pieces at their offsets add up to the same matrix
    seen = []
    r = cbg.MemEfficientSpGEMM_MCL(A, B, 3, *E2E, on_phase=lambda p, off, t: seen.append((p, off, t.to_host())))
    assert r is None and [s[0] for s in seen] == [0, 1, 2]
    from helpers import concat_cols_host
    assert [s[1] for s in seen] == [0, a["n"] // 3, 2 * (a["n"] // 3)]
    assert_tiles_bits_equal(concat_cols_host([s[2] for s in seen]), want)
    # all parameters zero: the unpruned product
    Z = cbg.MemEfficientSpGEMM_MCL(A, B, 3, 0.0, 0, 0, 0.0)
    assert_tiles_bits_equal(Z.tile.to_host(), C)
    assert cbg.mcl_stats()["pieces"] == 0
    with pytest.raises(cbg.CbgError) as e:
        cbg.MemEfficientSpGEMM_MCL(A, B, 3, 0.1, -1, 0, 0.0)
    assert e.value.code == cbg.INVALIDPARAMS
    with pytest.raises(ValueError):
        cbg.MemEfficientSpGEMM_MCL(A, B, 2, *E2E, on_phase=lambda p, off, t: (_ for _ in ()).throw(ValueError("x")))


def test_mcl_check_driver(cbg, tmp_path):
    """tools/mcl_check on the C++ mirror header: MemEfficientSpGEMM with pruning arguments,
    MCLPruneRecoverySelect, PruneColumn and Kselect; its pruned product of the scale-10
    matrix must have the digest of the restatement's."""
    exe = os.path.join(REPO, "tools", "mcl_check")
    if not os.path.exists(exe):
        pytest.fail("tools/mcl_check is not built (make -C combblas-spmm-test_amd drivers)")
    a, C, want, g = _product(10)
    mtx = str(tmp_path / "a.mtx")
    cbg.write_mm(mtx, a)
    from helpers import digest
    d = digest(want)
    r = subprocess.run([exe, mtx, repr(E2E[0]), str(E2E[1]), str(E2E[2]), repr(E2E[3])], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "MCLCHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"nnz {d['nnz']} hs {d['hs']} hv {d['hv']}" in r.stdout, (d, r.stdout[-1500:])


# ---------------------------------------------------------------------------
# several ranks on one GPU
# ---------------------------------------------------------------------------
def _launch(nproc, args, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(HERE, "mcl_worker.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = r.stdout + r.stderr
    errs = [ln for ln in out.splitlines() if "CbgError" in ln or "[cbg]" in ln or "AssertionError" in ln]
    return r.returncode, "\n".join(errs[:16]) + "\n" + out


@pytest.mark.parametrize("grid", [(2, 1), (1, 2), (2, 2)])
def test_mcl_multirank_host_transport(grid):
    """cbg_grid_kselect, cbg_grid_mcl_prune and MemEfficientSpGEMM_MCL on a grid, gathered,
    equal the 1 x 1 results (a column whose top k lie in one row block, a column empty on
    one rank, selection over the union of the ranks' multisets)."""
    rc, out = _launch(grid[0] * grid[1], ["gpu", str(grid[0]), str(grid[1])])
    assert rc == 0 and out.count("MCLOK") == grid[0] * grid[1], out[:1500] + out[-3000:]


def test_mcl_multirank_rccl():
    rc, out = _launch(2, ["rccl", "2", "1"])
    assert rc == 0 and out.count("MCLOK") == 2 and "transport rccl" in out, out[:1500] + out[-3000:]
