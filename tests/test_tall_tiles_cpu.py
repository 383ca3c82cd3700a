"""The tall-tile cases of tests/test_gpu_tall_tiles.py without a device: helpers.tall_operands builds
what its spec says, and helpers.tall_plan -- the documented rules of csrc/cbg_local.hip and
csrc/cbg_thin.hip restated on the host -- puts every B column on the route the case is meant to
hit.  The counts asserted here are worked out from the specs (helpers.tall_spec_*), not read off a
run: a change of the builder or of a rule that empties a route fails here, before the GPU test
could pass vacuously."""
import time

import numpy as np
import pytest

import helpers as H

G64 = {64: 0, 32: 0, 16: 0, 8: 0, 4: 0, 2: 0, 1: 0}


def _check_built(name):
    Ah, Bh, plan = H.tall_case(name)
    assert plan["routes"] == plan["intended"], list(zip(plan["routes"], plan["intended"]))
    assert H.digest(Ah)["unsorted"] == 0 and H.digest(Bh)["unsorted"] == 0
    assert Ah["ir"].min() >= 0 and int(Ah["ir"].max()) < Ah["m"]
    assert sum(plan["slabs"].values()) == plan["n_slabs"] == len(plan["slab_keys"])
    return Ah, Bh, plan


def test_rules_restated():
    """the predictor's pieces against the documented constants"""
    assert [H.tall_sparse_class(n, H.PANEL) for n in (683, 684, 1024, 1025, 2049)] == [
        "hash_T1536", "rank_N1024", "rank_N1024", "rank_N2048", "rank_N4096"]
    span = 1 << 22
    assert H.tall_sparse_class(684, span, 4096, group=True) == "group_rank_N2048"        # span 2^22: the <= edge
    assert H.tall_sparse_class(2049, span, 4096, group=True) == "group_rank_N4096"
    assert H.tall_sparse_class(684, span, 4097, group=True) == "hash_T1536"              # > 4096 products
    assert H.tall_sparse_class(684, 2 * span, 4096, group=True) == "hash_T1536"          # 32 panels
    assert H.tall_sparse_class(684, span + 5, 4096, group=True) == "hash_T1536"
    assert H.tall_sparse_class(4096, 64 * H.PANEL, 5461, group=True) == "hash_T6144"
    assert [H.thin_key_bits(m, n) for m, n in (((1 << 27), 32), ((1 << 27), 33), ((1 << 27) + 5, 16),
                                               ((1 << 27) + 5, 17), (H.TALL_MAX_M, 3), (H.TALL_MAX_M, 2))] == [
        32, 33, 32, 33, 33, 32]


def test_rows_without_an_array_of_m():
    """rows of a 2^31-row range: distinct, inside, the required ones among them"""
    rng = np.random.default_rng(1)
    must = [0, 5, H.TALL_MAX_M - 1]
    r = H._distinct_rows(rng, 0, H.TALL_MAX_M, 4000, must)
    assert len(np.unique(r)) == 4000 and r.min() == 0 and r.max() == H.TALL_MAX_M - 1 and 5 in r
    r = H._distinct_rows(rng, 1 << 27, (1 << 27) + 5, 5, [1 << 27])
    assert sorted(r) == list(range(1 << 27, (1 << 27) + 5))


def test_case_r65():
    """R = 65: three 64-panel-class columns (4160 and 4097 flops, the class's edges, and one with
    rows in panel 64 only), two 32-panel-class ones (4161 flops: the edge), each with panel 64
    as its own deferred unit"""
    Ah, Bh, p = _check_built("r65")
    assert p["R"] == 65 and list(p["flops"][:5]) == [4160, 4097, 4130, 4161, 8000]
    assert p["class_columns"] == {**G64, 64: 3, 32: 2} and p["n_big"] == 5
    assert (p["thin_columns"], p["esc_columns"], p["small_columns"], p["copy_columns"]) == (1, 1, 1, 1)
    assert p["thin_key_bits"] == 26
    assert (p["sym_group_units"], p["sym_panel_units"], p["sym_deferred_units"]) == (3 * 2 + 2 * 3, 0, 5)
    assert p["slabs"] == dict(hash_T3072=1, hash_T512=2, hash_T1536=3, bitmap_small=1, hash_T768=1, hash_T2048=1)
    g = p["groups"]
    assert g[0] == [(0, 63, 4110, 1500, "hash_T3072"), (64, 64, 50, 40, "deferred")]
    assert g[1] == [(0, 63, 4097, 700, "hash_T1536"), (64, 64, 0, 0, "deferred")]
    assert g[2] == [(0, 63, 0, 0, "empty"), (64, 64, 4130, 77, "deferred")]
    assert [x[4] for x in g[3]] == ["hash_T768", "hash_T1536", "deferred"]
    # the group's first and last row and the tile's last row are rows of A
    for r in (0, (1 << 24) - 1, 1 << 24, Ah["m"] - 1):
        assert r in Ah["ir"]


@pytest.mark.parametrize("name", ["r512", "r513"])
def test_case_r512_r513(name):
    """both sides of R = 512 | 513 (slab keys by class and panel | by class): one column per group
    class 64 .. 4, every group rank edge in the 16-panel class, the groups that leave the group
    path, and at R = 513 the 5-row panel 512 as every column's last, deferred, unit"""
    Ah, Bh, p = _check_built(name)
    R = p["R"]
    tail = R - 512
    assert R == {"r512": 512, "r513": 513}[name] and p["slab_keys_by_panel"] == (R == 512)
    big = [int(f) for f in p["flops"][:6]]
    assert big == [x + 10 * tail for x in (30000, 60000, 120000, 105173, 249600, 499200)]
    for F, g in zip(big, (64, 32, 16, 16, 8, 4)):     # in the upper half of the class's range, not thin
        top, below = 4096 * R // g, (4096 * R // (2 * g) if g < 64 else 4096)
        assert (top + below) / 2 < F <= top
    assert (4 * p["flops"][:6] >= p["entries"][:6] * R).all() and (p["entries"][:6] <= H.TALL_BIG_BS).all()
    assert p["class_columns"] == {**G64, 64: 1, 32: 1, 16: 2, 8: 1, 4: 1} and p["n_big"] == 6
    assert (p["thin_columns"], p["esc_columns"], p["small_columns"], p["copy_columns"]) == (0, 3, 3, 1)
    units = sum(-(-R // g) for g in (64, 32, 16, 16, 8, 4))
    assert units == (280 if R == 512 else 286)
    # deferred: groups 22, 24 and 25 of the second 16-panel column; at R = 513 every column's panel 512
    assert (p["sym_group_units"], p["sym_panel_units"], p["sym_deferred_units"]) == (units, 0, 3 + 6 * tail)
    # the deferred groups' 3 x 16 panels and the 6 ragged panels are small hash slabs
    assert p["slabs"] == dict(hash_T1536=8 + 16 + 8, group_rank_N2048=16 + 21 + 64, group_rank_N4096=8 + 128,
                              hash_T4096=1, hash_T6144=1, hash_T512=48 + 6 * tail)
    assert p["n_slabs"] == 319 + 6 * tail
    g16 = p["groups"][2]
    assert [x[4] for x in g16[:4]] == ["hash_T1536", "group_rank_N2048", "group_rank_N2048", "group_rank_N4096"]
    # a group rank slab spanning exactly 2^22 rows whose first row is 2^27 - 2^22
    assert g16[31][:2] == (496, 511) and g16[31][3] == 2049 and g16[31][4] == "group_rank_N4096"
    odd = p["groups"][3]
    assert [x[4] for x in odd[21:26]] == ["hash_T4096", "deferred", "hash_T6144", "deferred", "deferred"]
    assert all(x[4] == "empty" for x in odd[26:32])
    # 32- and 64-panel groups of more than 683 nonzeros are hash slabs
    assert all(x[3] > H.TALL_RANK_MIN and x[4] == "hash_T1536" for x in p["groups"][0][:8] + p["groups"][1][:16])
    # at least three slab classes in at least three panels each: the (class, panel) order has something to order
    panels = {}
    for cls, r in p["slab_keys"]:
        panels.setdefault(cls, set()).add(r)
    assert sum(1 for s in panels.values() if len(s) >= 3) >= 3, {k: len(v) for k, v in panels.items()}
    for r in (0, (1 << 27) - (1 << 22), (1 << 27) - 1, Ah["m"] - 1):
        assert r in Ah["ir"]


def test_case_r8192():
    """m = 2^31 - 2: three 64-panel-class columns of 128 groups, one group deferred into the last
    panel (a bitmap pair holding rows m - 2 and m - 1), three thin columns on 64-bit keys"""
    Ah, Bh, p = _check_built("r8192")
    m = H.TALL_MAX_M
    assert Ah["m"] == m and p["R"] == 8192 and not p["slab_keys_by_panel"] and Ah["n"] <= 2000
    assert [int(f) for f in p["flops"][:3]] == [99840, 82800, 99840]
    assert p["class_columns"] == {**G64, 64: 3} and p["n_big"] == 3
    assert (p["thin_columns"], p["esc_columns"], p["small_columns"], p["copy_columns"]) == (3, 3, 1, 2)
    assert p["thin_key_bits"] == 33
    assert (p["sym_group_units"], p["sym_panel_units"], p["sym_deferred_units"]) == (3 * 128, 0, 1)
    assert p["slabs"] == dict(hash_T1536=26 + 20, hash_T6144=26, bitmap_small=1) and p["n_slabs"] == 73
    assert p["groups"][1][127] == (8128, 8191, 6000, 2000, "deferred")
    assert ("bitmap_small", 8191) in p["slab_keys"]
    for r in (0, (1 << 31) - (1 << 18) - 1, (1 << 31) - (1 << 18), m - 2, m - 1):
        assert r in Ah["ir"]
    assert int(Ah["ir"].max()) == m - 1 and Ah["ir"].dtype == np.int32


@pytest.mark.parametrize("m,nthin", [(1 << 27, 33), ((1 << 27) + 5, 17)])
@pytest.mark.parametrize("arows", [2, 8])
def test_thin_key_cases(m, nthin, arows):
    """nthin thin columns are one past the 32-bit keys, nthin - 1 the last that fit; every column
    thin; the inline records of A are on for the columns of one or two rows only"""
    Ah, Bh = H.thin_key_operands(m, nthin, arows)
    p = H.tall_plan(Ah, Bh)
    assert p["routes"] == ["thin"] * nthin and p["thin_key_bits"] == 33
    assert H.thin_key_bits(m, nthin - 1) == 32
    assert H.tall_plan(Ah, H.split_cols_host(Bh, nthin - 1)[0])["thin_columns"] == nthin - 1
    nnzA, flops = len(Ah["ir"]), int(p["flops"].sum())
    inline = nnzA <= 2 * len(Ah["jc"]) and flops >= 4 * nnzA      # csrc/cbg_local.hip sym_small_columns
    assert inline == (arows == 2)
    for r in (0, (1 << 27) - 1, m - 1):
        assert r in Ah["ir"]
    C = H.oracle_local(Ah, Bh)
    assert len(C["ir"]) < flops // 2      # the products collide


def test_oracle_is_quick_on_every_case():
    """the oracle's cost is the products, not m: every case in a few seconds"""
    for name in ("r65", "r512", "r513", "r8192"):
        Ah, Bh, p = H.tall_case(name)
        t = time.perf_counter()
        C = H.oracle_local(Ah, Bh)
        dt = time.perf_counter() - t
        print(name, "products", int(p["flops"].sum()), "nnz(C)", len(C["ir"]), "%.2f s" % dt)
        assert H.digest(C)["unsorted"] == 0 and C["m"] == Ah["m"]
        assert dt < 5.0
