"""Staged runs of the big columns (csrc/cbg_local.hip, SymPanelArgs::runs): the symbolic of a
bitmap-mode (column, panel) pair writes every B entry's run of A(:,k) inside the panel, and
the numeric's bitmap slabs (k_num_slab<..., RUNS>) read them instead of hopping through A's
panel map.  All or nothing per multiply; CBG_STAGE_RUNS=0 keeps the hops, CBG_STAGE_RUNS_CAP
(bytes) is the budget's test hook.

Every case runs under both settings and requires equal C (bit for bit), equal flops and nnz
and every other work counter equal, and compares C with the CPU oracle or the golden digests."""
import functools

import numpy as np
import pytest

import helpers as H
from helpers import abs_tile, assert_digest_eq, assert_tiles_bits_equal, assert_tiles_equal, golden, oracle_local

pytestmark = pytest.mark.gpu

RTOL = 1e-12
STAGED = ("staged_multiplies", "staged_entries")
M = (1 << 20) + 77  # 5 row panels of 2^18, the last one partial


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for k in ("CBG_STAGE_RUNS", "CBG_STAGE_RUNS_CAP", "CBG_BIG_FLOPS", "CBG_CUTS_CAP", "CBG_THIN"):
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def _panel():
    return H.panel_group_operands(M)


@functools.lru_cache(maxsize=None)
def _panel_wide():
    """_panel()'s A with a B of two columns of 800 and 1300 entries over the 100-row A columns
    (the first 3000): more B entries than one staging chunk of the symbolic (512), and pairs
    of two and three bitmap slabs, whose inner slabs take cuts at both ends"""
    rng = np.random.default_rng(31)
    Ah, _ = _panel()
    bcols = [np.sort(rng.choice(3000, nb, replace=False)) for nb in (800, 1300)]
    bc = np.array([len(c) for c in bcols])
    Bh = dict(m=Ah["n"], n=2, cp=np.concatenate([[0], np.cumsum(bc)]).astype(np.int64), jc=np.arange(2, dtype=np.int32),
              ir=np.concatenate(bcols).astype(np.int32), val=rng.integers(1, 3, int(bc.sum())).astype(np.float64))
    return Ah, Bh


@functools.lru_cache(maxsize=None)
def _uniform(name):
    """the operands with U[-1, 1) values: no exact int32 accumulation, (row, f64) records"""
    rng = np.random.default_rng(37)
    Ah, Bh = OPERANDS[name]()
    A, B = dict(Ah), dict(Bh)
    A["val"] = rng.uniform(-1.0, 1.0, len(Ah["ir"]))
    B["val"] = rng.uniform(-1.0, 1.0, len(Bh["ir"]))
    return A, B


OPERANDS = {"panel": _panel, "wide": _panel_wide}


@functools.lru_cache(maxsize=None)
def _reference(name, values, sr):
    Ah, Bh = OPERANDS[name]() if values == "int" else _uniform(name)
    ref = oracle_local(Ah, Bh, sr)
    bound = oracle_local(abs_tile(Ah), abs_tile(Bh))["val"] if (values, sr) == ("uniform", "plus") else None
    return ref, bound


def _multiply(cbg, Ah, Bh, sr):
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    C = cbg.LocalHybridSpGEMM(A, B, sr)
    st, w = cbg.last_stats(), {k: int(v) for k, v in cbg.last_work_stats().items()}
    Ch = C.to_host()
    for t in (A, B, C):
        t.free()
    return Ch, st, w


def _both(cbg, monkeypatch, Ah, Bh, sr, expect_staged=True):
    """the multiply with staged runs and with the map hops: equal C by bits, equal flops and
    nnz, every other work counter equal; returns the staged run's (C, counters)"""
    C1, st1, w1 = _multiply(cbg, Ah, Bh, sr)
    monkeypatch.setenv("CBG_STAGE_RUNS", "0")
    C0, st0, w0 = _multiply(cbg, Ah, Bh, sr)
    monkeypatch.delenv("CBG_STAGE_RUNS")
    print(sr, st1["n_big"], {k: v for k, v in w1.items() if v})
    assert w0["staged_multiplies"] == 0 and w0["staged_entries"] == 0, w0
    if expect_staged:
        assert w1["staged_multiplies"] == 1 and w1["staged_entries"] > 0, w1
        assert w1["bitmap_small_kept"] + w1["bitmap_large_kept"] + w1["bitmap_small_mark"] + w1["bitmap_large_mark"] > 0
    assert (st1["flops"], st1["nnz"], st1["n_big"], st1["n_slabs"]) == (st0["flops"], st0["nnz"], st0["n_big"],
                                                                      st0["n_slabs"])
    assert {k: v for k, v in w1.items() if k not in STAGED} == {k: v for k, v in w0.items() if k not in STAGED}
    assert_tiles_bits_equal(C1, C0)
    return C1, w1


@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("name", ["panel", "wide"])
def test_staged_runs_vs_oracle(cbg, monkeypatch, name, sr):
    """every big-column class of helpers.panel_group_operands() (bitmap pairs, hash pairs, panel
    groups and their per-panel fallbacks, which stage runs from k_sym_deferred), and the two wide
    columns: entry for entry against the oracle (integer values: exact in any order)"""
    Ah, Bh = OPERANDS[name]()
    C, w = _both(cbg, monkeypatch, Ah, Bh, sr)
    assert_tiles_equal(C, _reference(name, "int", sr)[0])
    if name == "wide":
        # 5 panels x 2 columns; the pairs of the full panels hold more than one slab
        assert w["staged_entries"] == 5 * (800 + 1300), w
        assert w["bitmap_large_kept"] + w["bitmap_large_mark"] > 10, w


def test_wide_columns_expected_counts():
    """the wide columns' sizes, checked with numpy: about 19.2 K / 30.5 K nonzeros per full
    panel (two / three slabs of at most 12032) and a handful in the last panel of 77 rows"""
    Ah, Bh = _panel_wide()
    for j, (lo, hi, slabs) in enumerate([(18500, 20000, 2), (29500, 31500, 3)]):
        ks = Bh["ir"][Bh["cp"][j]:Bh["cp"][j + 1]]
        rows = np.unique(np.concatenate([Ah["ir"][Ah["cp"][k]:Ah["cp"][k + 1]] for k in ks]))
        per = np.bincount(rows >> 18, minlength=5)
        assert np.all((per[:4] > lo) & (per[:4] < hi)) and 0 < per[4] < 16, per
        assert np.all(-(-per[:4] // 12032) == slabs), per


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_staged_runs_meet_searched_cuts(cbg, monkeypatch, sr):
    """CBG_CUTS_CAP=0: the multi-slab pairs' cuts are searched by the numeric inside the staged runs"""
    monkeypatch.setenv("CBG_CUTS_CAP", "0")
    Ah, Bh = _panel_wide()
    C, w = _both(cbg, monkeypatch, Ah, Bh, sr)
    assert_tiles_equal(C, _reference("wide", "int", sr)[0])


@pytest.mark.parametrize("name", ["panel", "wide"])
def test_staged_runs_random_values(cbg, monkeypatch, name):
    """U[-1, 1) values (no int32 accumulation, (row, f64) records): 1e-12 (|A||B|)ij"""
    Ah, Bh = _uniform(name)
    for sr in ("plus", "minplus"):
        C1, st1, w1 = _multiply(cbg, Ah, Bh, sr)
        monkeypatch.setenv("CBG_STAGE_RUNS", "0")
        C0, st0, w0 = _multiply(cbg, Ah, Bh, sr)
        monkeypatch.delenv("CBG_STAGE_RUNS")
        assert w1["staged_multiplies"] == 1 and w0["staged_multiplies"] == 0 and w1["int_accumulate"] == 0, (w1, w0)
        assert {k: v for k, v in w1.items() if k not in STAGED} == {k: v for k, v in w0.items() if k not in STAGED}
        ref, bound = _reference(name, "uniform", sr)
        for C in (C1, C0):
            if sr == "plus":
                assert_tiles_equal(C, ref, rtol=RTOL, bound=bound)
            else:
                assert_tiles_equal(C, ref)


@pytest.mark.parametrize("big", [None, "64"])
@pytest.mark.parametrize("scale", [12, 14])
def test_staged_runs_rmat_digests(cbg, monkeypatch, scale, big):
    """R-MAT (one row panel, multi-slab hub columns) against the golden digests"""
    if big:
        monkeypatch.setenv("CBG_BIG_FLOPS", big)
    g = golden()["rmat"][f"s{scale}_ef16"]
    for sr, key in (("plus", "C_local_plus"), ("minplus", "C_local_minplus")):
        ws = []
        for setting in (None, "0"):
            if setting:
                monkeypatch.setenv("CBG_STAGE_RUNS", setting)
            A, B = cbg.rmat_tile(scale, 16), cbg.rmat_tile(scale, 16)
            C = cbg.LocalHybridSpGEMM(A, B, sr)
            ws.append({k: int(v) for k, v in cbg.last_work_stats().items()})
            assert_digest_eq(C.digest(), g[key])
            assert cbg.last_stats()["flops"] == g["symbolic"]["flops"]
            for t in (A, B, C):
                t.free()
            monkeypatch.delenv("CBG_STAGE_RUNS", raising=False)
        # scale 12 under the default cut: its big columns (above 4096 flops) hold a quarter of
        # B's entries, below the half the staged runs ask for
        want = 0 if (scale, big) == (12, None) else 1
        assert ws[0]["staged_multiplies"] == want and (ws[0]["staged_entries"] > 0) == bool(want), ws
        assert ws[1]["staged_multiplies"] == 0 and ws[1]["staged_entries"] == 0, ws
        assert {k: v for k, v in ws[0].items() if k not in STAGED} == {k: v for k, v in ws[1].items() if k not in STAGED}


def test_budget_too_small_falls_back_whole(cbg, monkeypatch):
    """a budget below the buffer (B's entries x 5 panels x 8 B): the multiply runs with the map
    hops, the counters say so, and C is the same"""
    Ah, Bh = _panel()
    need = int(Bh["cp"][-1]) * 5 * 8
    C1, _, w1 = _multiply(cbg, Ah, Bh, "plus")
    monkeypatch.setenv("CBG_STAGE_RUNS_CAP", str(need - 1))
    C0, _, w0 = _multiply(cbg, Ah, Bh, "plus")
    monkeypatch.setenv("CBG_STAGE_RUNS_CAP", str(need))
    C2, _, w2 = _multiply(cbg, Ah, Bh, "plus")
    assert w1["staged_multiplies"] == 1 and w2["staged_multiplies"] == 1 and w2["staged_entries"] == w1["staged_entries"]
    assert w0["staged_multiplies"] == 0 and w0["staged_entries"] == 0, w0
    assert {k: v for k, v in w1.items() if k not in STAGED} == {k: v for k, v in w0.items() if k not in STAGED}
    assert_tiles_bits_equal(C0, C1)
    assert_tiles_bits_equal(C2, C1)
    assert_tiles_equal(C1, _reference("panel", "int", "plus")[0])


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def _piece_expectation(lo, hi):
    """(cut, B entries of the big columns) of the piece B(:, lo:hi) of the scale-14 R-MAT square,
    from the oracle's flops per column: the lower-cut rule of tests/test_gpu_group_count.py, and
    at R = 1 every big column is one bitmap-mode pair (more than 1024 products against the 256 a
    sparse pair may have), so the piece's staged entries are its big columns' B entries"""
    A = H.oracle_rmat(14, 16)
    f = np.asarray(H.oracle_symbolic(A, dict(A))[0], np.int64)
    nb, jc = np.diff(A["cp"]), np.asarray(A["jc"])
    sel = (jc >= lo) & (jc < hi)
    f, nb = f[sel], nb[sel]
    low = 2 * int(f[(f > 4096) & (nb > 1)].sum()) >= int(f.sum()) and int(((f > 1024) & (f <= 4096) & (nb > 1)).sum()) > 0
    cut = 1024 if low else 4096
    big = (f > cut) & (nb > 1)
    return cut, int(nb[big].sum()), int(nb.sum())


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_two_phase_pieces_stage_their_own_runs(cbg, monkeypatch, sr):
    """MemEfficientSpGEMM of the scale-14 square in two column pieces of B, unlike in their
    columns, entries and big-column entries: the buffer is the piece's (sized by and indexed with
    the piece's own B positions), never the A-side state the call caches across its pieces -- every
    piece reports its own big columns' entries as staged, the pieces' digests add up to the golden
    one, and the hops give the same digests and the same other counters piece by piece"""
    g = golden()["rmat"]["s14_ef16"]["C_local_plus" if sr == "plus" else "C_local_minplus"]
    runs = {}
    for setting in (None, "0"):
        if setting:
            monkeypatch.setenv("CBG_STAGE_RUNS", setting)
        grid = _self_grid(cbg)
        nv = 1 << 14
        A = cbg.SpParMat(cbg.rmat_tile(14, 16), grid, nv, nv)
        B = cbg.SpParMat(cbg.rmat_tile(14, 16), grid, nv, nv)
        parts, prev = [], {}

        def on_phase(ph, off, t):
            w = {k: int(v) for k, v in cbg.last_work_stats().items()}
            d = {k: v - prev.get(k, 0) for k, v in w.items()}
            d["big_cut_flops"] = w["big_cut_flops"]  # (not a sum: the last multiply's)
            prev.clear()
            prev.update(w)
            parts.append((ph, off, t.n, t.digest(0, off), d))

        try:
            cbg.MemEfficientSpGEMM(A, B, 2, sr, on_phase=on_phase)
        finally:
            A.tile.free()
            B.tile.free()
            grid.destroy()
        monkeypatch.delenv("CBG_STAGE_RUNS", raising=False)
        runs[setting] = parts
    staged, hops = runs[None], runs["0"]
    assert [p[0] for p in staged] == [0, 1] == [p[0] for p in hops]
    total = dict(nnz=0, hs=0, hv=0)
    seen = []
    for (ph, off, n, d, w), (ph0, off0, n0, d0, w0) in zip(staged, hops):
        cut, big_entries, entries = _piece_expectation(off, off + n)
        print(ph, off, n, cut, big_entries, entries, {k: v for k, v in w.items() if v})
        assert (off, n) == (off0, n0) and d == d0 and d["unsorted"] == 0
        assert w["big_cut_flops"] == cut and 2 * big_entries >= entries
        assert w["staged_multiplies"] == 1 and w["staged_entries"] == big_entries, (w, big_entries)
        assert w0["staged_multiplies"] == 0 and w0["staged_entries"] == 0, w0
        assert {k: v for k, v in w.items() if k not in STAGED} == {k: v for k, v in w0.items() if k not in STAGED}
        # the cached A-side state is what the second piece reuses; the runs are not part of it
        if ph == 1:
            assert w["amap_reused"] == 1 and w["pmap_reused"] == 1, w
        seen.append((n, entries, big_entries))
        total["nnz"] += d["nnz"]
        total["hs"] += int(d["hs"], 16)
        total["hv"] += int(d["hv"], 16)
    assert seen[0] != seen[1]  # unlike pieces
    assert (total["nnz"], "%016x" % (total["hs"] % (1 << 64)), "%016x" % (total["hv"] % (1 << 64))) == \
        (g["nnz"], g["hs"], g["hv"])
