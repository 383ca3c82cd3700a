"""The CPU oracle (oracle/cbg_oracle.c) is pinned against the reference's own outputs
(tests/golden/, produced by oracle/_ref/ref_driver linked with the reference sources)."""
import numpy as np
import pytest

from helpers import (assert_digest_eq, assert_tiles_bits_equal, assert_tiles_equal, digest, golden, load_npz,
                     oracle_local, oracle_rmat, oracle_summa, oracle_symbolic, oracle_edges, abs_tile)
import helpers as H

G = golden()


@pytest.mark.parametrize("scale", [8, 10, 12, 14, 16])
def test_rmat_generator_matches_reference(scale):
    A = oracle_rmat(scale, 16)
    g = G["rmat"][f"s{scale}_ef16"]["A"]
    assert_digest_eq(digest(A), g)
    assert digest(A)["nzc"] == g["nzc"]


@pytest.mark.parametrize("scale", [8, 10])
def test_rmat_full_tile(scale):
    A = oracle_rmat(scale, 16)
    R = load_npz(f"rmat_s{scale}_ef16_A.npz")
    assert_tiles_equal(A, R)


@pytest.mark.parametrize("scale", [8, 10, 12, 14])
@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_local_hybrid_matches_reference(scale, sr):
    A = oracle_rmat(scale, 16)
    C = oracle_local(A, A, sr)
    assert_digest_eq(digest(C), G["rmat"][f"s{scale}_ef16"][f"C_local_{sr}"])


@pytest.mark.parametrize("scale", [8, 10])
def test_local_full_product(scale):
    A = oracle_rmat(scale, 16)
    for sr in ("plus", "minplus"):
        C = oracle_local(A, A, sr)
        assert_tiles_equal(C, load_npz(f"rmat_s{scale}_ef16_C_local_{sr}.npz"))


@pytest.mark.parametrize("algo", ["doublebuff", "synch"])
@pytest.mark.parametrize("scale", [8, 12])
def test_summa_1x1_and_2x2(algo, scale):
    A = oracle_rmat(scale, 16)
    g = G["rmat"][f"s{scale}_ef16"]
    C1 = oracle_summa(A, A, 1, algo)
    assert_digest_eq(digest(C1), g[f"C_{algo}_plus"])
    if algo == "doublebuff":
        C2 = oracle_summa(A, A, 2, algo)
        d = digest(C2)
        assert d["nnz"] == g["C_doublebuff_plus_p4"]["nnz"] and d["hv"] == g["C_doublebuff_plus_p4"]["hv"]


def test_heap_equals_hybrid():
    A = oracle_rmat(10, 16)
    assert_tiles_equal(oracle_local(A, A, heap=True), oracle_local(A, A))


def test_symbolic_totals():
    A = oracle_rmat(12, 16)
    f, n = oracle_symbolic(A, A)
    s = G["rmat"]["s12_ef16"]["symbolic"]
    assert int(f.sum()) == s["flops"] and int(n.sum()) == s["nnzC"] and int(n.max()) == s["maxcol"]


@pytest.mark.parametrize("name", ["sevenvertex", "small_nonsym", "largeseq"])
@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_bundled_inputs(name, sr):
    A = load_npz(f"{name}_A.npz")
    B = load_npz(f"{name}_B.npz") if name == "largeseq" else A
    ref = load_npz(f"{name}_C_local_{sr}.npz")
    C = oracle_local(A, B, sr)
    if sr == "plus":
        bound = oracle_local(abs_tile(A), abs_tile(B), "plus")["val"]
        assert_tiles_equal(C, ref, rtol=1e-12, bound=bound)
    else:
        assert_tiles_equal(C, ref)  # min-plus is exact
    for algo in ("doublebuff", "synch"):
        Cs = oracle_summa(A, B, 1, algo, sr)
        assert_tiles_equal(Cs, ref, rtol=1e-12, bound=np.abs(ref["val"]) + 1e-300 if sr == "minplus" else bound)


def test_edge_prefix_is_rank_independent():
    # Global edge ids are independent of the partition (RefGen21::compute_edge_range, RefGen21.h:263-269)
    s0, d0 = oracle_edges(10, 0, 4096)
    s1, d1 = oracle_edges(10, 1000, 2000)
    np.testing.assert_array_equal(s0[1000:2000], s1)
    np.testing.assert_array_equal(d0[1000:2000], d1)


# ---- bit-level comparison, value palettes and boundary operands (tests/test_gpu_value_bits.py) ----
def _one(vals):
    n = len(vals)
    return dict(m=n, n=1, cp=np.array([0, n], np.int64), jc=np.zeros(1, np.int32), ir=np.arange(n, dtype=np.int32),
                val=np.array(vals, np.float64))


def test_bits_helper_sees_zero_sign_and_nan():
    assert_tiles_equal(_one([1.0, -0.0]), _one([1.0, 0.0]))  # the value comparison cannot tell them apart
    with pytest.raises(AssertionError, match="8000000000000000"):
        assert_tiles_bits_equal(_one([1.0, -0.0]), _one([1.0, 0.0]))
    with pytest.raises(AssertionError):
        assert_tiles_bits_equal(_one([1.0, np.nan]), _one([1.0, 2.0]))
    with pytest.raises(AssertionError):
        assert_tiles_bits_equal(_one([1.0, 2.0]), _one([1.0, np.nan]))
    quiet = np.array([0x7FF8000000000000, 0xFFF8000000000123], np.uint64).view(np.float64)
    assert_tiles_bits_equal(_one([quiet[0], -0.0, np.inf]), _one([quiet[1], -0.0, np.inf]))  # NaN: by position
    with pytest.raises(AssertionError):
        assert_tiles_bits_equal(_one([np.inf]), _one([H.DBL_MAX]))
    with pytest.raises(AssertionError):  # structure first
        assert_tiles_bits_equal(_one([1.0, 2.0]), dict(_one([1.0, 2.0]), ir=np.array([0, 2], np.int32)))


@pytest.mark.parametrize("palette", sorted(H.PALETTES))
def test_palette_products_do_not_depend_on_order(palette):
    """the oracle's hash path and its heap path add in different orders: with the row-class
    palettes they agree bit for bit, and the special values are there (NaN < 10 %, and
    -0.0 >= 1 % of nnz(C) where the palette holds zeros)"""
    Ah, Bh = H.rand_hub_operands(0)
    A, B = H.with_palette(Ah, Bh, palette, np.random.default_rng(17))
    p = H.PALETTES[palette]
    assert set(np.unique(A["val"]).tolist()) <= {v for c in p["A"] for v in c}
    for sr in (("plus", "minplus") if p["sr"] == "both" else (p["sr"],)):
        C = oracle_local(A, B, sr)
        assert_tiles_bits_equal(oracle_local(A, B, sr, heap=True), C)
        if sr == "plus":
            H.assert_palette_not_vacuous(C, palette)
        else:
            assert not np.isnan(C["val"]).any() and not (np.signbit(C["val"]) & (C["val"] == 0)).any()
    if palette == "f32":
        assert np.array_equal(A["val"].astype(np.float32).astype(np.float64), A["val"])
    if palette == "f64":
        with np.errstate(over="ignore"):
            assert not np.array_equal(A["val"].astype(np.float32).astype(np.float64), A["val"])
    if palette == "minplus":
        for v in (np.inf, H.DBL_MAX, -H.DBL_MAX):
            assert (C["val"] == v).any(), v


@pytest.mark.parametrize("m,layout,mixed", [(5000, "dense", False), (5000, "dense", True),
                                            ((1 << 20) + 77, "random", True), ((1 << 20) + 77, "stride128", False),
                                            ((1 << 20) + 77, "edges", True)])
def test_boundary_operands_hit_their_table(m, layout, mixed):
    """precondition of the GPU bin-boundary sweep: every B column has exactly the intended
    (flops, nnz), and the sweep holds t-1, t, t+1 of every threshold"""
    Ah, Bh, table = H.boundary_operands(m, layout, "plus", mixed)
    f, z = oracle_symbolic(Ah, Bh)
    assert [(int(a), int(b)) for a, b in zip(f, z)] == table
    fs, zs = {t[0] for t in table}, {t[1] for t in table}
    for t in H.SYM_THR:
        assert {t - 1, t, t + 1} <= fs and {(t, t), (t + 1, t + 1), (t - 1, t - 1)} <= set(table)
    for t in H.NUM_THR:
        assert {t - 1, t, t + 1} <= zs
    if layout == "edges":
        assert set(H.panel_edge_rows(m).tolist()) <= set(Ah["ir"].tolist())
    if layout == "stride128":
        assert not (Ah["ir"] & 127).any()


@pytest.mark.parametrize("m", [1 << 18, (1 << 18) + 1, 3 << 18, (1 << 21) + 1])
def test_panel_edge_operands(m):
    bd = H.panel_edge_rows(m)
    assert {0, 31, 32, 63, 64, m - 2, m - 1} <= set(bd.tolist()) and bd.max() == m - 1
    for p in range(1, (m - 1) // H.PANEL + 1):
        assert {p * H.PANEL - 1, p * H.PANEL} <= set(bd.tolist())
    Ah, Bh = H.panel_edge_operands(m)
    f, _ = oracle_symbolic(Ah, Bh)
    assert f.min() > H.BIG_FLOPS  # every B column is a big column
    for j in range(len(Ah["jc"])):  # every A column holds every boundary row
        assert np.isin(bd, Ah["ir"][Ah["cp"][j]:Ah["cp"][j + 1]]).all()


def test_host_restatements_of_tile_ops():
    A = oracle_rmat(8, 16)
    L, R = H.split_cols_host(A, 100)
    assert_tiles_bits_equal(H.concat_cols_host([L, R]), A)
    T, Bm = H.split_rows_host(A, 77)
    assert len(T["ir"]) + len(Bm["ir"]) == len(A["ir"]) and T["ir"].max() < 77 and Bm["m"] == A["m"] - 77
    assert_tiles_bits_equal(H.transpose_host(H.transpose_host(A)), A)


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_special_values_match_reference(sr):
    """signed zeros, infinities, inf * 0 and inf - inf NaNs, subnormals, the DBL_MAX
    sentinel: the oracle's hash and heap paths against the reference's own C
    (tests/golden/make_golden.py special), bit for bit"""
    A, B = load_npz(f"special_{sr}_A.npz"), load_npz(f"special_{sr}_B.npz")
    ref = load_npz(f"special_{sr}_C_local.npz")
    nan, negz = H.special_shares(ref)
    if sr == "plus":
        assert 0 < nan < 0.10 and negz >= 0.01 and np.isinf(ref["val"]).any()
    else:
        assert (ref["val"] == H.DBL_MAX).any() and np.isinf(ref["val"]).any()
    for heap in (False, True):
        assert_tiles_bits_equal(oracle_local(A, B, sr, heap=heap), ref)
