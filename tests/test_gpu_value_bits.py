"""The local multiply and everything built on it, compared with the CPU oracle by the
value BITS (tests/helpers.py assert_tiles_bits_equal: -0.0 is not +0.0, NaN by position),
on values no other test holds -- signed zeros, infinities, the NaN of inf * 0 and
inf - inf, f32 and f64 subnormals, magnitudes outside f32's range, min-plus's DBL_MAX
sentinel and its +inf "empty slot" -- and on columns placed exactly on the dispatch
thresholds and rows exactly on the panel and bitmap-word edges.

Bit equality needs a C that does not depend on the accumulation order: the palettes
(helpers.PALETTES) let A's value depend on the class of its row, so every C entry combines
products of one class, and all sums are exact, or inf / NaN in any order.  The oracle itself
is pinned to the reference on such values in tests/test_oracle.py
(test_special_values_match_reference)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from helpers import assert_tiles_bits_equal, oracle_local, oracle_symbolic

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))


# --------------------------------------------------------------------------
# special values through every kernel family
# --------------------------------------------------------------------------
def _rmat14():
    A = H.oracle_rmat(14, 16)
    return A, dict(A)


STRUCTURES = {
    "esc": lambda: H.esc_operands(5000),            # expand-sort-compress waves
    "single": H.single_entry_operands,              # scaled copies, small and big
    "thin": H.thin_operands,                        # the thin-column pass
    "panel": H.panel_group_operands,                # m = 2^20 + 77: panel groups, hash pairs, bitmap pairs, fallbacks
    "rmat14": _rmat14,                              # bitmap and rank slabs
    "hub": lambda: H.rand_hub_operands(0),          # wave / block hash bins
}
PALETTE_SR = [(p, sr) for p in ("f32", "f64", "int0", "int", "minplus")
              for sr in (("plus", "minplus") if H.PALETTES[p]["sr"] == "both" else (H.PALETTES[p]["sr"],))]
_WORK = {}   # (palette, structure, sr) -> last_work_stats() of that multiply


@functools.lru_cache(maxsize=None)
def _structure(name):
    return STRUCTURES[name]()


def _operands(palette, structure):
    Ah, Bh = _structure(structure)
    return H.with_palette(Ah, Bh, palette, np.random.default_rng(17))


def _multiply(cbg, palette, structure, sr):
    """the multiply on the device: C on the host, and its work statistics remembered"""
    Ah, Bh = _operands(palette, structure)
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    C = cbg.LocalHybridSpGEMM(A, B, sr)
    w = {k: int(v) for k, v in cbg.last_work_stats().items()}
    _WORK[(palette, structure, sr)] = w
    Ch = C.to_host()
    for t in (A, B, C):
        t.free()
    print(palette, structure, sr, {k: v for k, v in w.items() if v})
    return Ah, Bh, Ch, w


@pytest.mark.parametrize("structure", sorted(STRUCTURES))
@pytest.mark.parametrize("palette,sr", PALETTE_SR)
def test_special_values_bit_exact(cbg, palette, sr, structure):
    Ah, Bh, C, w = _multiply(cbg, palette, structure, sr)
    ref = oracle_local(Ah, Bh, sr)
    if sr == "plus":
        print("NaN and -0.0 share of nnz(C):", H.assert_palette_not_vacuous(ref, palette))
    else:
        assert not np.isnan(ref["val"]).any()
    assert_tiles_bits_equal(C, ref)
    # exact int32 accumulation: never with a zero in A or B (int cannot carry -0.0)
    if palette != "int":
        assert w["int_accumulate"] == 0, w
    elif structure in ("panel", "rmat14"):
        assert w["int_accumulate"] > 0, w


def _summed(palette, srs, cbg):
    tot = {}
    for structure in sorted(STRUCTURES):
        for sr in srs:
            w = _WORK.get((palette, structure, sr)) or _multiply(cbg, palette, structure, sr)[3]
            for k, v in w.items():
                tot[k] = tot.get(k, 0) + v
    return tot


@pytest.mark.parametrize("palette", ["f32", "f64", "int0", "int", "minplus"])
def test_special_values_reached_every_family(cbg, palette):
    """the structures of one palette, taken together, ran every kernel family (the
    multiplies of test_special_values_bit_exact; one not run in this session is run here)"""
    srs = [sr for p, sr in PALETTE_SR if p == palette]
    w = _summed(palette, srs, cbg)
    fam = dict(bitmap_kept=[k for k in w if k.startswith("bitmap_") and k.endswith("_kept")],
               rank=[k for k in w if k.startswith("rank_N")], group_rank=[k for k in w if k.startswith("group_rank_N")],
               hash=[k for k in w if k.startswith("hash_T")])
    for name, keys in fam.items():
        assert sum(w[k] for k in keys) > 0, (name, w)
    for k in ("esc_columns", "thin_columns", "single_big_entries", "hash_bin_columns", "wave_bin_columns",
              "sym_panel_units", "sym_group_units"):
        assert w[k] > 0, (k, w)


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_int_accumulate_rank_slabs(cbg, sr):
    """the int32 instantiations of the rank and group-rank slab kernels run, with negative
    values and in both semirings: over the `int` palette's multi-panel (m = 2^20 + 77) and
    scale-14 multiplies alone, every multiply accumulates in int32 and some rank and some
    group-rank class is used (bit equality: test_special_values_bit_exact)"""
    tot = {}
    for structure in ("panel", "rmat14"):
        w = _WORK.get(("int", structure, sr)) or _multiply(cbg, "int", structure, sr)[3]
        assert w["int_accumulate"] > 0, (structure, w)
        for k, v in w.items():
            tot[k] = tot.get(k, 0) + v
    assert sum(v for k, v in tot.items() if k.startswith("rank_N")) > 0, tot
    assert sum(v for k, v in tot.items() if k.startswith("group_rank_N")) > 0, tot


def _sub(code, env, timeout=300):
    """run `code` in a fresh process (the knobs in `env` are read once per process);
    its last line of output is JSON"""
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path.insert(0, %r)\n" % TESTS + code],
                       capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_special_values_marking_pass():
    """no kept bitmaps (CBG_BITMAP_BUDGET_GB=0): the numeric's own marking pass, f64 palette
    on R-MAT scale 14"""
    code = r'''
import json
import numpy as np
from conftest import load_cbg
import helpers as H
cbg = load_cbg()
A0 = H.oracle_rmat(14, 16)
Ah, Bh = H.with_palette(A0, dict(A0), "f64", np.random.default_rng(17))
C = cbg.LocalHybridSpGEMM(cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh))
w = {k: int(v) for k, v in cbg.last_work_stats().items()}
ref = H.oracle_local(Ah, Bh)
H.assert_palette_not_vacuous(ref, "f64")
H.assert_tiles_bits_equal(C.to_host(), ref)
print(json.dumps(w))
'''
    w = _sub(code, {"CBG_BITMAP_BUDGET_GB": "0"})
    assert w["bitmap_small_mark"] + w["bitmap_large_mark"] > 0, w
    assert w["bitmap_small_kept"] + w["bitmap_large_kept"] == 0, w


# --------------------------------------------------------------------------
# merge, SUMMA and the pass-through operations keep the bits
# --------------------------------------------------------------------------
@pytest.mark.parametrize("palette", ["f32", "f64"])
def test_merge_plus_keeps_bits(cbg, palette):
    """A split by columns, B by rows: the two partial products merged are the full product,
    bit for bit (a -0.0 held by one partial only stays -0.0)"""
    Ah, Bh = _operands(palette, "hub")
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    A1, A2 = A.split_cols(A.n // 2)
    B1, B2 = B.split_rows(B.m // 2)
    P1, P2 = cbg.LocalHybridSpGEMM(A1, B1), cbg.LocalHybridSpGEMM(A2, B2)
    one = P1.to_host()
    assert (np.signbit(one["val"]) & (one["val"] == 0)).any()  # a partial does hold -0.0
    C = cbg.MergeAll([P1, P2]).to_host()
    ref = oracle_local(Ah, Bh)
    H.assert_palette_not_vacuous(ref, palette)
    assert_tiles_bits_equal(C, ref)


_MERGE_CODE = r'''
import json
from conftest import load_cbg
import helpers as H
cbg = load_cbg()
parts, want = H.merge_minplus_parts()
C = cbg.MergeAll([cbg.Tile.from_dict(p) for p in parts], "minplus").to_host()
H.assert_tiles_bits_equal(C, want)
print(json.dumps(cbg.merge_stats()))
'''


def test_merge_minplus_keeps_bits(cbg):
    """min-plus MergeAll of host-built partials: an entry held by one partial comes out
    unchanged (-0.0, +0.0, +inf, DBL_MAX, a subnormal), a shared one as the minimum"""
    parts, want = H.merge_minplus_parts()
    v = np.concatenate([p["val"] for p in parts])
    assert (np.signbit(v) & (v == 0)).any() and (~np.signbit(v) & (v == 0)).any() and np.isinf(v).any()
    assert len(want["ir"]) < len(v)  # shared positions exist
    assert (np.signbit(want["val"]) & (want["val"] == 0)).sum() > 100
    C = cbg.MergeAll([cbg.Tile.from_dict(p) for p in parts], "minplus").to_host()
    assert_tiles_bits_equal(C, want)


def test_merge_minplus_chunked_keeps_bits():
    """the same through the column-chunked merge (CBG_MERGE_CHUNK, read once per process)"""
    ms = _sub(_MERGE_CODE, {"CBG_MERGE_CHUNK": "5000"})
    assert ms["entries_in"] > ms["entries_out"] > 0


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def test_summa_keeps_bits(cbg):
    """Mult_AnXBn_Synch / _DoubleBuff and MemEfficientSpGEMM with 3 phases on the 1x1 grid,
    f64 palette"""
    Ah, Bh = _operands("f64", "hub")
    ref = oracle_local(Ah, Bh)
    H.assert_palette_not_vacuous(ref, "f64")
    g = _self_grid(cbg)
    A = cbg.SpParMat(cbg.Tile.from_dict(Ah), g, Ah["m"], Ah["n"])
    B = cbg.SpParMat(cbg.Tile.from_dict(Bh), g, Bh["m"], Bh["n"])
    for f in (cbg.Mult_AnXBn_Synch, cbg.Mult_AnXBn_DoubleBuff, lambda a, b: cbg.MemEfficientSpGEMM(a, b, 3)):
        C = f(A, B)
        assert_tiles_bits_equal(C.tile.to_host(), ref)
        C.tile.free()
    g.destroy()


def test_pass_through_ops_keep_bits(cbg):
    """upload / download, split_cols, split_rows, column concatenation and Transpose move
    values: every bit stays (NaN payloads included: nothing is computed)"""
    Ah, _ = _operands("f64", "hub")
    Ah = dict(Ah, val=Ah["val"].copy())
    Ah["val"][::11] = np.array([0x7FF8000000000001, 0xFFF0000000000000, 0x0000000000000001, 0x8000000000000000,
                                0x7FEFFFFFFFFFFFFF], np.uint64).view(np.float64)[np.arange(len(Ah["val"][::11])) % 5]

    def same(t, want):
        h = t.to_host()
        assert_tiles_bits_equal(h, want)
        np.testing.assert_array_equal(h["val"].view(np.uint64), want["val"].view(np.uint64))  # NaN bits too

    A = cbg.Tile.from_dict(Ah)
    same(A, Ah)
    cut = Ah["n"] // 3
    L, R = A.split_cols(cut)
    Lh, Rh = H.split_cols_host(Ah, cut)
    same(L, Lh)
    same(R, Rh)
    same(cbg.Tile.concat_cols([L, R]), Ah)
    rc = Ah["m"] // 2 + 1
    T, Bm = A.split_rows(rc)
    Th, Bh = H.split_rows_host(Ah, rc)
    same(T, Th)
    same(Bm, Bh)
    same(A.transpose(), H.transpose_host(Ah))
    A.Transpose()
    A.Transpose()
    same(A, Ah)


# --------------------------------------------------------------------------
# bin boundaries
# --------------------------------------------------------------------------
BOUNDARY_LAYOUTS = [(5000, "dense", False), (5000, "dense", True), ((1 << 20) + 77, "random", True),
                    ((1 << 20) + 77, "stride128", False), ((1 << 20) + 77, "edges", True)]


def _expected_big_and_thin(m, table, nb_of, big):
    """k_classify's rule (csrc/cbg_local.hip): a column of more than `big` flops and more than
    one B entry is a big column, unless (R >= 4 row panels) flops * 4 < B entries * R: thin"""
    R = (m + H.PANEL - 1) // H.PANEL
    n_big = n_thin = 0
    for (f, _), nb in zip(table, nb_of):
        if f > big and nb > 1:
            thin = R >= 4 and f * 4 < nb * R
            n_thin += thin
            n_big += not thin
    return n_big, n_thin


@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("m,layout,mixed", BOUNDARY_LAYOUTS)
def test_bin_boundaries(cbg, m, layout, mixed, sr):
    """B columns at t-1, t, t+1 of every flops threshold (kSymThr, full table nnz = flops and
    half-full) and of every nnz threshold (kNumThr), 4096 / 4097 flops around the big-column
    threshold; rows nearly dense, random, on a stride of 128 (all low hash bits zero) or packed
    around the panel edges"""
    Ah, Bh, table = H.boundary_operands(m, layout, sr, mixed)
    f, z = oracle_symbolic(Ah, Bh)  # precondition, on the CPU: the columns are what they claim
    assert [(int(a), int(b)) for a, b in zip(f, z)] == table
    assert {(4096, 4096), (4097, 4097), (4095, 4095)} <= set(table)
    C = cbg.LocalHybridSpGEMM(cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh), sr)
    st, w = cbg.last_stats(), cbg.last_work_stats()
    print({k: int(v) for k, v in w.items() if v}, st["n_big"])
    assert_tiles_bits_equal(C.to_host(), oracle_local(Ah, Bh, sr))
    n_big, n_thin = _expected_big_and_thin(m, table, np.diff(Bh["cp"]), H.BIG_FLOPS)
    assert n_big + n_thin == sum(3 for t in set(table) if t[0] > 4096) > 0  # f = 4097 counts, f = 4096 does not
    assert st["n_big"] == n_big and w["thin_columns"] == n_thin, (st, n_big, n_thin)
    assert st["flops"] == int(f.sum()) and st["nnz"] == int(z.sum())


def test_bin_boundaries_big_flops_64():
    """the big-column threshold moved to 64 (CBG_BIG_FLOPS, read once per process): 64 flops
    is a small column, 65 a big one"""
    code = r'''
import json
import numpy as np
from conftest import load_cbg
import helpers as H
cbg = load_cbg()
pairs = [p for p in H.boundary_pairs() if p[0] <= 300]
out = {}
for sr in ("plus", "minplus"):
    Ah, Bh, table = H.boundary_operands(5000, "dense", sr, True, pairs=pairs)
    C = cbg.LocalHybridSpGEMM(cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh), sr)
    n_big = cbg.last_stats()["n_big"]
    H.assert_tiles_bits_equal(C.to_host(), H.oracle_local(Ah, Bh, sr))
    out[sr] = dict(n_big=n_big, want=sum(1 for (f, z), nb in zip(table, np.diff(Bh["cp"])) if f > 64 and nb > 1),
                   at64=sum(1 for f, z in table if f == 64), at65=sum(1 for f, z in table if f == 65))
print(json.dumps(out))
'''
    out = _sub(code, {"CBG_BIG_FLOPS": "64"})
    for sr in ("plus", "minplus"):
        o = out[sr]
        assert o["at64"] > 0 and o["at65"] > 0 and o["n_big"] == o["want"] > o["at65"], out


# --------------------------------------------------------------------------
# panel- and word-boundary rows in big columns
# --------------------------------------------------------------------------
@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("m", [1 << 18, (1 << 18) + 1, 3 << 18, (1 << 21) + 1])
def test_panel_edge_rows_in_big_columns(cbg, m, sr):
    """every A column holds the rows 0, 31, 32, 63, 64, m-2, m-1 and p 2^18 - 1, p 2^18,
    p 2^18 + 1 of every panel edge; all B columns are big columns (slab kernels), one of them
    made of boundary rows only; m with a full last panel, a last panel of one row, three
    panels, eight panels and one row"""
    Ah, Bh = H.panel_edge_operands(m, sr)
    C = cbg.LocalHybridSpGEMM(cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh), sr)
    st, w = cbg.last_stats(), cbg.last_work_stats()
    print({k: int(v) for k, v in w.items() if v}, st["n_big"])
    assert st["n_big"] == Bh["n"]
    ref = oracle_local(Ah, Bh, sr)
    bd = H.panel_edge_rows(m)
    for j in range(Bh["n"]):  # every column of C holds every boundary row
        assert np.isin(bd, ref["ir"][ref["cp"][j]:ref["cp"][j + 1]]).all()
    assert_tiles_bits_equal(C.to_host(), ref)
    slab = sum(v for k, v in w.items() if k.startswith(("bitmap_", "rank_N")))
    multi = sum(v for k, v in w.items() if k.startswith(("group_rank_N", "hash_T")))
    assert slab + multi > 0, w
    if m > (1 << 18) + 1:
        assert slab > 0 and multi > 0, w
    else:
        assert slab > 0, w


# --------------------------------------------------------------------------
# cbg_local_symbolic
# --------------------------------------------------------------------------
def _symbolic_cases():
    yield "boundary_dense", lambda: H.boundary_operands(5000, "dense", "plus", True)[:2]
    yield "boundary_edges", lambda: H.boundary_operands((1 << 20) + 77, "edges", "plus", True)[:2]
    yield "panel_edges", lambda: H.panel_edge_operands((1 << 21) + 1)
    yield "rmat12", lambda: (H.oracle_rmat(12, 16), H.oracle_rmat(12, 16))


@pytest.mark.parametrize("name,make", list(_symbolic_cases()), ids=[n for n, _ in _symbolic_cases()])
def test_local_symbolic(cbg, name, make):
    """LocalSymbolic (cbg_local_symbolic: flops and nnz(C) without forming C) = the oracle's
    per-column counts summed = what the real multiply reports"""
    Ah, Bh = make()
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    f, z = oracle_symbolic(Ah, Bh)
    assert cbg.LocalSymbolic(A, B) == (int(f.sum()), int(z.sum()))
    C = cbg.LocalHybridSpGEMM(A, B)
    st = cbg.last_stats()
    assert (st["flops"], st["nnz"]) == (int(f.sum()), int(z.sum())) and C.nnz == st["nnz"]
    if name == "rmat12":
        s = H.golden()["rmat"]["s12_ef16"]["symbolic"]
        assert (st["flops"], st["nnz"]) == (s["flops"], s["nnzC"])


def test_local_symbolic_edge_cases(cbg):
    E = dict(m=5, n=4, cp=np.zeros(1, np.int64), jc=np.zeros(0, np.int32), ir=np.zeros(0, np.int32), val=np.zeros(0))
    X = dict(m=4, n=3, cp=np.array([0, 2], np.int64), jc=np.array([1], np.int32), ir=np.array([0, 3], np.int32),
             val=np.array([1.0, -1.0]))
    assert cbg.LocalSymbolic(cbg.Tile.from_dict(E), cbg.Tile.from_dict(X)) == (0, 0)  # empty A
    with pytest.raises(cbg.CbgError) as e:
        cbg.LocalSymbolic(cbg.Tile.from_dict(X), cbg.Tile.from_dict(X))  # 4 x 3 times 4 x 3
    assert e.value.code == cbg.DIMMISMATCH
