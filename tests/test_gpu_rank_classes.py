"""Every launch class of the rank slabs (csrc/cbg_local.hip k_num_slab_rank: rank_N1024 / N2048 /
N4096) and of the group rank slabs (k_num_slab_grank: group_rank_N2048 / N4096), with the hash
class below their lower bound of 684 nonzeros.

A B column selects a few A columns; within one unit -- a row panel (rank slabs) or a group of
two panels (group rank slabs) -- the first of them holds N distinct rows and the others subsets
of those rows, so the unit's slab has exactly N nonzeros, sums of products, and a chosen number
of products in (2048, 4096] (N = 4096: two A columns of 2048 of the rows each, 4096 products
and no sums).  Every B column has two such units, hence more than 4096 flops: a
big column under either cut (big_cut_flops is asserted, since the lower cut takes its columns in
whole-column groups).  C is compared with oracle_local by bits (integers and half-integers:
exact in any order); the route is read from last_work_stats()."""
import functools

import numpy as np
import pytest

import helpers as H
from helpers import assert_tiles_bits_equal, oracle_local
from test_gpu_slab_lds import multiply

pytestmark = pytest.mark.gpu

PANEL = 1 << 18
RANK_MIN = 683          # csrc/cbg_local.hip RANK_SLABS_MIN, GRANK_SLABS_MIN: slabs of more nonzeros are ranked
HASH_T = (512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192)
RANK = ("rank_N1024", "rank_N2048", "rank_N4096")
GRANK = ("group_rank_N2048", "group_rank_N4096")
NCOLS = 3               # B columns of one multiply: 2 * NCOLS slabs of the class
ENV = ("CBG_BIG_FLOPS", "CBG_GROUPS", "CBG_GRANK_MIN", "CBG_THIN", "CBG_STAGE_RUNS", "CBG_STAGE_RUNS_CAP", "CBG_DBG")

# rows every unit holds, relative to the unit's first row
# rank slabs: the panel's first and last row, both sides of a 128-row edge (4 bitmap words are
# one group prefix) near either end
RANK_ROWS = np.array([0, 127, 128, PANEL - 129, PANEL - 128, PANEL - 1], np.int64)
# group rank slabs: both ends of the 2^19-row span, both sides of a 32-row block edge (a level-1
# bit), of a 1024-row edge (a level-1 word) and of the edge between the group's two panels
SPAN = 2 * PANEL
GRANK_ROWS = np.array([0, 31, 32, 1023, 1024, PANEL - 1, PANEL, SPAN - 1025, SPAN - 1024, SPAN - 33, SPAN - 32,
                       SPAN - 1], np.int64)


@pytest.fixture(autouse=True)
def _no_overrides(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def expected_class(n, ranked):
    """the launch class of a sparse slab of n nonzeros: `ranked` (the rank or the group rank
    classes, by their bounds) above RANK_MIN, else the smallest hash table of load <= 2/3"""
    if n > RANK_MIN:
        return next(k for k in ranked if n <= int(k.rsplit("N", 1)[1]))
    return "hash_T%d" % next(t for t in HASH_T if 2 * t >= 3 * n)


def subset_sizes(n):
    """sizes of the A columns of one unit after the first (n rows): products in (2048, 4096]"""
    if n > 2048:
        return [min(n, 4096 - n)] if n < 4096 else []
    out = []
    while n + sum(out) <= 2100:
        out.append(min(n, 700))
    return out


def operands(n, span, must, values, negate, seed):
    """A (2 * span rows): for B column c and j = 0, 1, ... the column holding, in either unit
    u = 0, 1, rows u * span + (`must` and random others: n of them for j = 0, a subset for
    j > 0); B: column c = its A columns.  values `int`: integers 1..4 in A and 1..2 in B;
    `half`: the same with A's values + 0.5 (f32-exact, not integral: the f64 slabs)."""
    rng = np.random.default_rng(seed)
    sizes = subset_sizes(n)
    products = n + sum(sizes)
    assert 2048 < products <= 4096 and len(must) <= min([n] + sizes)
    pool = np.setdiff1d(np.arange(span), must)
    acols, bcols = [], []
    for c in range(NCOLS):
        units = []
        for u in range(2):
            rows = np.concatenate([must, rng.choice(pool, n - len(must), replace=False)])
            rest = np.setdiff1d(rows, must)
            if sizes:
                units.append([rows] + [np.concatenate([must, rng.choice(rest, z - len(must), replace=False)])
                                       for z in sizes])
            else:  # 4096 products are the n = 4096 rows once: two A columns of half of them each
                units.append([rows[:n // 2], rows[n // 2:]])  # (a B column of one entry is copied, not multiplied)
        ncol = len(units[0])
        bcols.append(np.arange(len(acols), len(acols) + ncol))
        acols += [np.sort(np.concatenate([units[0][j], span + units[1][j]])) for j in range(ncol)]
    na = sum(len(c) for c in acols)
    assert na == 2 * NCOLS * products
    av = rng.integers(1, 5, na).astype(np.float64) + (0.5 if values == "half" else 0.0)
    Ah = H.dcsc_from_cols(2 * span, len(acols), acols, -av if negate else av)
    Bh = H.dcsc_from_cols(len(acols), NCOLS, bcols, rng.integers(1, 3, sum(len(b) for b in bcols)).astype(np.float64))
    return Ah, Bh


@functools.lru_cache(maxsize=None)
def _case(n, span, values, negate, sr):
    Ah, Bh = operands(n, span, RANK_ROWS if span == PANEL else GRANK_ROWS, values, negate, seed=n)
    return Ah, Bh, oracle_local(Ah, Bh, sr)


def check_case(cbg, n, span, ranked, values, negate, sr):
    Ah, Bh, ref = _case(n, span, values, negate, sr)
    C, w, st = multiply(cbg, Ah, Bh, sr)
    want = expected_class(n, ranked)
    print("n", n, "want", want, {k: v for k, v in w.items() if v})
    assert len(C["ir"]) == 2 * NCOLS * n
    assert_tiles_bits_equal(C, ref)
    assert w["big_cut_flops"] == 4096 and st["n_big"] == NCOLS and st["n_slabs"] == 2 * NCOLS, (n, st, w)
    assert w["int_accumulate"] == int(values == "int"), (n, w)
    got = {k: w[k] for k in RANK + GRANK + tuple("hash_T%d" % t for t in HASH_T) if w[k]}
    assert got == {want: 2 * NCOLS}, (n, want, got)
    assert sum(w[k] for k in w if k.startswith("bitmap_")) == 0 and w["thin_columns"] == 0, (n, w)
    # single-panel units for the rank slabs, groups of two panels for the group rank slabs
    units = ("sym_panel_units", "sym_group_units") if span == PANEL else ("sym_group_units", "sym_panel_units")
    assert w[units[0]] == 2 * NCOLS and w[units[1]] == 0 and w["sym_deferred_units"] == 0, (n, w)


def test_expected_classes():
    """the prediction itself, without a multiply: the classes' bounds (csrc/cbg_local.hip slab_class)"""
    assert [expected_class(n, RANK) for n in (683, 684, 1024, 1025, 2048, 2049, 4096)] == [
        "hash_T1536", "rank_N1024", "rank_N1024", "rank_N2048", "rank_N2048", "rank_N4096", "rank_N4096"]
    assert [expected_class(n, GRANK) for n in (683, 684, 2048, 2049, 4096)] == [
        "hash_T1536", "group_rank_N2048", "group_rank_N2048", "group_rank_N4096", "group_rank_N4096"]
    for n in (683, 684, 1024, 1025, 2048, 2049, 4096):
        assert 2048 < n + sum(subset_sizes(n)) <= 4096


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("values", ["int", "half"])
def test_rank_classes(cbg, values, sr, negate):
    """m = 2 * 2^18 (two row panels): every (column, panel) pair is a single-panel unit of N
    nonzeros and <= 4096 products -- 683 a hash slab, 684 and 1024 rank_N1024, 1025 and 2048
    rank_N2048, 2049 and 4096 rank_N4096"""
    for n in (683, 684, 1024, 1025, 2048, 2049, 4096):
        check_case(cbg, n, PANEL, RANK, values, negate, sr)


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("values", ["int", "half"])
def test_group_rank_classes(cbg, values, sr, negate):
    """m = 2^20 (four row panels), column flops in (4096, 8192]: the column is taken in groups
    of two panels, each of N nonzeros over its 2^19 rows and <= 4096 products -- 683 a hash
    slab, 684 and 2048 group_rank_N2048, 2049 and 4096 group_rank_N4096"""
    for n in (683, 684, 2048, 2049, 4096):
        check_case(cbg, n, SPAN, GRANK, values, negate, sr)
