"""The local multiply on tall tiles: the switches that depend on the number of row panels
R = ceil(m / 2^18) or on m itself (csrc/cbg_local.hip, csrc/cbg_thin.hip), each with real work
on both of its sides at the smallest size that reaches it.

  r65     m = 2^24 + 77: the 64-panel group class (4097..4160 flops), its slab over 2^24 rows, the
          lone ragged panel 64 as a deferred unit, a column with rows in panel 64 only; 32-panel
          groups beside them
  r512    m = 2^27 (slab list keyed by class and panel) and r513, m = 2^27 + 5 (by class alone): the
          same spec, one column per group class 64 .. 4; group rank slabs at every edge of their
          classes, spanning exactly 2^22 rows up to a first row of 2^27 - 2^22; 32- and 64-panel
          groups of more than 683 nonzeros (hash slabs); groups that leave the group path
  thin    32 | 33 thin columns at m = 2^27 and 16 | 17 at 2^27 + 5: 32- | 64-bit (column, row) keys
  r8192   m = 2^31 - 2, the tallest tile the ABI admits: 64-panel groups, a bitmap pair in the
          last panel (rows m - 2, m - 1), thin columns on 31 row bits, ESC and copy columns

Every C is compared with oracle_local: by bits under the `int` (IACC) and `half` (f64 slabs)
values, exact in any summation order, for plus-times and min-plus; within RTOL (|A||B|)_ij under
random values.  The route is read from last_stats() / last_work_stats() and set against
helpers.tall_plan, whose expectations tests/test_tall_tiles_cpu.py pins without a device.

The counters' rules (k_sym_panel, sym_group, sym_big_columns; restated in tall_plan): a column of
group class g counts ceil(R / g) units, empty ones too; a group unit is deferred -- run panel by
panel by k_sym_deferred -- when it is one panel (the ragged last group, empty or not), or has more
than 5461 products, or more than 4096 nonzeros; any other nonempty group is one sparse slab."""
import numpy as np
import pytest

import helpers as H
from helpers import abs_tile, assert_tiles_bits_equal, assert_tiles_equal, oracle_local

pytestmark = pytest.mark.gpu

RTOL = 1e-12            # tests/test_gpu_local.py: |dC| <= RTOL (|A||B|)_ij
ENV = ("CBG_BIG_FLOPS", "CBG_GRANK_MIN", "CBG_THIN", "CBG_STAGE_RUNS", "CBG_STAGE_RUNS_CAP", "CBG_CUTS_CAP", "CBG_DBG")
SLAB_KEYS = (["hash_T%d" % t for t in H.TALL_HASH_T] + ["rank_N1024", "rank_N2048", "rank_N4096",
                                                         "group_rank_N2048", "group_rank_N4096"])
BITMAP = ("bitmap_small_kept", "bitmap_small_mark", "bitmap_large_kept", "bitmap_large_mark")


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def multiply(cbg, Ah, Bh, sr):
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    try:
        C = cbg.LocalHybridSpGEMM(A, B, sr)
        w = {k: int(v) for k, v in cbg.last_work_stats().items()}
        st = cbg.last_stats()
        Ch = C.to_host()
        C.free()
    finally:
        A.free()
        B.free()
    return Ch, w, st


def check_route(tag, plan, w, st, iacc):
    """the multiply's counters against the plan: the cut, the big and thin columns, the symbolic's
    units, and every slab class (which sum to n_slabs)"""
    print(tag, "n_big", st["n_big"], "n_slabs", st["n_slabs"], {k: v for k, v in w.items() if v})
    assert w["big_cut_flops"] == H.BIG_FLOPS, w
    assert st["n_big"] == plan["n_big"] and w["thin_columns"] == plan["thin_columns"], (st, w)
    assert w["esc_columns"] == plan["esc_columns"], w
    assert w["int_accumulate"] == int(iacc and plan["n_big"] > 0), w
    if plan["n_big"] == 0:
        assert st["n_slabs"] == 0 and sum(w[k] for k in SLAB_KEYS + list(BITMAP)) == 0, (st, w)
        return
    for k in ("sym_group_units", "sym_panel_units", "sym_deferred_units"):
        assert w[k] == plan[k], (k, w[k], plan[k])
    got = {k: w[k] for k in SLAB_KEYS if w[k]}
    for k in ("bitmap_small", "bitmap_large"):
        if w[k + "_kept"] + w[k + "_mark"]:
            got[k] = w[k + "_kept"] + w[k + "_mark"]
    assert got == plan["slabs"], (got, plan["slabs"])
    assert sum(got.values()) == st["n_slabs"] == plan["n_slabs"], (got, st)
    assert w["slab_over_cap"] == 0, w


def run_case(cbg, name):
    """the case under both exact value sets and both semirings, by bits; once under random values"""
    plan = H.tall_case(name)[2]
    for values in ("int", "half"):
        for sr in ("plus", "minplus"):
            A, B, ref = H.tall_reference(name, values, sr)
            C, w, st = multiply(cbg, A, B, sr)
            check_route((name, values, sr), plan, w, st, values == "int")
            assert_tiles_bits_equal(C, ref)
    A, B, ref = H.tall_reference(name, "random", "plus")
    C, w, st = multiply(cbg, A, B, "plus")
    check_route((name, "random", "plus"), plan, w, st, False)
    assert_tiles_equal(C, ref, rtol=RTOL, bound=oracle_local(abs_tile(A), abs_tile(B))["val"])
    return plan


def test_64_panel_class_65_panels(cbg):
    """a. R = 65: columns of 4160 and 4097 flops in the 64-panel class (one slab over 2^24 rows and
    the ragged panel 64 deferred, also where it is empty), one whose only rows are panel 64's
    (an empty group; 4130 products on 77 rows: a bitmap pair), 4161 and 8000 flops in the
    32-panel class"""
    plan = run_case(cbg, "r65")
    assert plan["class_columns"][64] == 3 and plan["class_columns"][32] == 2


@pytest.mark.parametrize("name", ["r512", "r513"])
def test_group_classes_around_512_panels(cbg, name):
    """b. the same spec at m = 2^27 and 2^27 + 5, either side of the slab list's (class, panel)
    keys: a column per group class 64, 32, 16, 8, 4; group rank slabs of 684, 2048 and 2049
    nonzeros and a hash slab of 683 over exactly 2^22 rows, the last starting at row
    2^27 - 2^22; hash slabs for the 32- and 64-panel groups; groups of 4500 products (no group
    rank), 5461 products and 4096 nonzeros (the largest the group path takes), 5462 products
    and 4097 nonzeros (deferred); ESC, block-hash and copy columns beside them"""
    plan = run_case(cbg, name)
    assert plan["slabs"]["group_rank_N2048"] > 0 and plan["slabs"]["group_rank_N4096"] > 0
    assert plan["slab_keys_by_panel"] == (name == "r512")


@pytest.mark.parametrize("arows", [2, 8])
@pytest.mark.parametrize("m,n32", [(1 << 27, 32), ((1 << 27) + 5, 16)])
def test_thin_key_width(cbg, m, n32, arows):
    """c. n32 thin columns are the most that 32-bit keys hold at this m, n32 + 1 take the 64-bit
    instantiation (expand, sort, reduce-by-key, k_thin_rows); A's columns of one or two rows
    (the inline records) and of 8 rows; rows from a pool of 1500 with 0, 2^27 - 1 and m - 1.
    Both runs against the oracle by bits, and the columns they share bit for bit alike."""
    Ah, B64 = H.thin_key_operands(m, n32 + 1, arows)
    B32 = H.split_cols_host(B64, n32)[0]
    assert H.thin_key_bits(m, n32) == 32 and H.thin_key_bits(m, n32 + 1) == 33
    for sr in ("plus", "minplus"):
        got = []
        for Bh, n in ((B32, n32), (B64, n32 + 1)):
            plan = H.tall_plan(Ah, Bh)
            assert plan["thin_columns"] == n and plan["thin_key_bits"] == (32 if n == n32 else 33)
            C, w, st = multiply(cbg, Ah, Bh, sr)
            check_route((m, n, arows, sr), plan, w, st, True)
            assert_tiles_bits_equal(C, oracle_local(Ah, Bh, sr))
            got.append(C)
        assert_tiles_bits_equal(H.split_cols_host(got[1], n32)[0], got[0])


def test_tallest_tile(cbg):
    """d. m = 2^31 - 2 (R = 8192): three 64-panel-class columns (128 groups each; one group deferred
    into the last panel, whose bitmap pair holds rows m - 2 and m - 1 in a fine range that ends past
    2^31), three thin columns (31 row bits: 64-bit keys), ESC, block-hash and single-entry
    columns; rows 0, 2^31 - 2^18 - 1, m - 2, m - 1.  Device memory: the panel map is
    R x (n + 1) x 8 B = 31 MB, the kept bitmaps 3 x R x 32 KiB = 805 MB."""
    plan = run_case(cbg, "r8192")
    assert plan["thin_key_bits"] == 33 and plan["slabs"]["bitmap_small"] == 1


def test_tallest_tile_round_trip(cbg):
    """e. upload and download of the m = 2^31 - 2 operands and of their product keep every bit;
    the device's digest is the host's and counts no order violation"""
    A, B, ref = H.tall_reference("r8192", "half", "plus")
    for t in (A, B, ref):
        T = cbg.Tile.from_dict(t)
        try:
            back, d = T.to_host(), T.digest()
        finally:
            T.free()
        assert back["ir"].dtype == np.int32 and back["cp"].dtype == np.int64
        assert_tiles_bits_equal(back, t)
        h = H.digest(t)
        assert d["unsorted"] == 0 and (d["nnz"], d["nzc"], d["hs"], d["hv"]) == (h["nnz"], h["nzc"], h["hs"], h["hv"])
    assert int(A["ir"].max()) == H.TALL_MAX_M - 1 and int(ref["ir"].max()) == H.TALL_MAX_M - 1
