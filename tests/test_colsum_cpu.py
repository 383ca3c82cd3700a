"""The order-exact restatement of the column reductions (tests/colsum_ref.py) on the host:
its accuracy against math.fsum under a derived bound, exactness on dyadic inputs, and
non-vacuity -- on the very inputs the GPU tests use it differs by bits from every other
order a kernel could plausibly take, so a GPU test that matches it by bits pins the order."""
import math
from fractions import Fraction

import numpy as np
import pytest

import colsum_ref as cr
import hipmcl_ref as hr

U = 2.0 ** -53
CLASSES = (16, 64, 256)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _cols(t):
    """(length, values, rows) of every stored column"""
    return [(int(b - a), t["val"][a:b], t["ir"][a:b]) for a, b in zip(t["cp"][:-1], t["cp"][1:])]


def _depth(ln):
    """D = ceil(len / G) - 1 + log2 G, plus 3 for the block class: no entry passes through more
    additions than its lane's chain, the tree and the wave sums together"""
    g = cr.lanes_of(ln)
    return -(-ln // g) - 1 + int(math.log2(g)) + (3 if g == 256 else 0)


def test_classes():
    assert [cr.lanes_of(n) for n in (0, 1, 16, 17, 4096, 4097, 30000)] == [16, 16, 16, 64, 64, 256, 256]
    assert (cr.GROUP_MAX, cr.WAVE_MAX) == (16, 4096)
    for pattern in cr.PATTERNS:
        t = cr.inexact_case(pattern)
        lens = np.diff(t["cp"])
        assert sorted(set(lens.tolist())) == sorted(cr.LENGTHS) and t["m"] <= 16384
        assert len(np.setdiff1d(np.arange(t["n"]), t["jc"])) > 0
        assert all(np.all(np.diff(r) > 0) for _, _, r in _cols(t))
    assert np.all(cr.inexact_case("uniform")["val"] > 0) and np.any(cr.inexact_case("normal")["val"] < 0)
    w = cr.inexact_case("wide")["val"]
    assert w.min() < 1e-12 and w.max() > 1e12


@pytest.mark.parametrize("pattern", cr.PATTERNS)
def test_ordered_sums_within_the_derived_bound_of_fsum(pattern):
    """every entry passes through at most D additions, each with relative error <= u, so
    |ordered - exact| <= gamma_D sum|v|, gamma_D = D u / (1 - D u) (Higham, Accuracy and
    Stability of Numerical Algorithms, 4.2).  D counts the block class's tree as log2 256 = 8
    levels where it has 6.  fsum is the exact sum rounded once; that rounding (u |sum|) gets no
    allowance of its own: the bound is held as it stands.  The rounded squares are the elements
    of sumsq's sum; against the exact squares they carry one more rounding each"""
    worst = 0.0
    for ln, v, _ in _cols(cr.inexact_case(pattern)):
        d = _depth(ln)
        gam = d * U / (1 - d * U)
        mag = math.fsum(np.abs(v))
        err = abs(cr.ordered_sum(v) - math.fsum(v))
        assert err <= gam * mag, (pattern, ln, err, gam * mag)
        worst = max(worst, err / (gam * mag))
        sq = v * v
        gam1 = (d + 1) * U / (1 - (d + 1) * U)
        exact = sum(Fraction(x) ** 2 for x in v.tolist()) if ln <= 130 else None
        if exact is not None:
            assert abs(Fraction(cr.ordered_sumsq(v)) - exact) <= Fraction(gam1) * exact, (pattern, ln)
        assert abs(cr.ordered_sumsq(v) - math.fsum(sq)) <= gam * math.fsum(sq), (pattern, ln)
        assert cr.ordered_max(v) == max(v.tolist()) and cr.ordered_count(v) == ln
    print("largest error / bound, %s: %.3f" % (pattern, worst))
    assert worst > 0.0  # the inputs are inexact: some sum is rounded


def test_exact_on_dyadic_inputs():
    t = cr.inexact_case("dyadic", 4)
    for ln, v, r in _cols(t):
        assert _bits([cr.ordered_sum(v)])[0] == _bits([np.sum(v) + 0.0])[0], ln
        assert _bits([cr.ordered_sumsq(v)])[0] == _bits([np.sum(v * v)])[0], ln
        keep = v > np.sort(v)[ln // 2]
        assert cr.ordered_sum(v, keep) == np.sum(v[keep])
        for cuts in ([t["m"] // 2], [100, 5000, 12000]):
            assert cr.col_moment(v, r, "sum", cuts) == np.sum(v)
            assert cr.col_moment(v, r, "count", cuts) == ln and cr.col_moment(v, r, "max", cuts) == v.max()
    for what in ("sum", "sumsq", "max", "count"):
        for ident in (0.0, -7.5):
            np.testing.assert_array_equal(cr.reduce_cols_ordered(t, what, ident) + 0.0, hr.reduce_cols(t, what, ident) + 0.0)
    pos = dict(t, val=np.abs(t["val"]) + 1.0 / 1024)
    np.testing.assert_array_equal(_bits(cr.make_col_stochastic_ordered(pos)["val"]), _bits(hr.make_col_stochastic(pos)["val"]))
    assert cr.chaos_ordered(pos) == hr.chaos(pos)


def test_small_hand_cases():
    assert cr.ordered_sum([]) == 0.0 and cr.ordered_max([]) == -np.inf and cr.ordered_count([]) == 0.0
    assert _bits([cr.ordered_sum([-0.0, -0.0])])[0] == 0  # the lanes start at +0.0
    # 17 entries: a wave; lane 0 holds entry 0 only, lane 16 entry 16 -- not lane 0 (16 lanes would chain 0 and 16)
    v = np.array([1.0] + [2.0 ** -53] * 16)
    assert cr.ordered_sum(v) == 1.0 + 2.0 ** -49 and cr.lane_sum(v, lanes=16) == 1.0 + 2.0 ** -50 + 2.0 ** -52 * 3
    # a skipped entry leaves its lane as it was
    assert cr.ordered_sum([1.0, 2.0, 4.0], [True, False, True]) == 5.0
    assert cr.ordered_max([1.0, 9.0, 4.0], [True, False, True]) == 4.0
    assert cr.combine_ranks([0.0, 1.5, 2.5]) == 4.0 and cr.combine_ranks([-np.inf, 3.0, -np.inf], "max") == 3.0
    e = 2.0 ** -53  # ((1 + e) + e) + e = 1, (e + e) + (e + 1) = 1 + 2^-52: rank order shows
    assert cr.combine_ranks([1.0, e, e, e]) == 1.0 and cr.combine_ranks([e, e, e, 1.0]) > 1.0
    t = hr.from_coo(8, 4, [0, 3, 1, 2, 5], [1, 1, 2, 2, 2], [0.0, 0.0, 0.25, 0.5, 0.25])
    got, c = cr.inflate_ordered(t)
    np.testing.assert_array_equal(got["val"], [0.0, 0.0, 1 / 6, 4 / 6, 1 / 6])
    assert c == (0.5 - 0.375) * 3 == cr.chaos_ordered(cr.make_col_stochastic_ordered(t))
    assert cr.chaos_ordered(dict(t, val=np.array([np.inf, 1.0, 0.25, 0.5, 0.25]))) == (0.5 - 0.375) * 3  # NaN ignored


# ---------------------------------------------------------------------------
# non-vacuity: on the GPU tests' own inputs the restatement differs from its mutants
# ---------------------------------------------------------------------------
def _fma_sumsq(v):
    """ordered_sumsq with the lane's step contracted: acc = fma(v, v, acc), one rounding"""
    g = cr.lanes_of(len(v))
    acc = [0.0] * g
    for i, x in enumerate(v.tolist()):
        acc[i % g] = float(Fraction(x) * Fraction(x) + Fraction(acc[i % g]))
    return cr.lane_sum(np.asarray(acc), lanes=g)  # one round: every lane holds its finished partial


def _differs(t, mutant, restated=cr.ordered_sum):
    """per length: in how many columns the mutant's bits differ from the restatement's"""
    out = {}
    for ln, v, _ in _cols(t):
        out[ln] = out.get(ln, 0) + int(_bits([restated(v)])[0] != _bits([mutant(v)])[0])
    return out


def _lengths_of_class(g, lo=1):
    return [ln for ln in cr.LENGTHS if cr.lanes_of(ln) == g and ln >= lo]


@pytest.mark.parametrize("pattern", cr.PATTERNS)
def test_order_mutants_differ(pattern):
    t = cr.inexact_case(pattern)
    # a plain host sum: every class with at least three entries
    d = _differs(t, lambda v: float(np.sum(v)))
    for g in CLASSES:
        assert any(d[ln] for ln in _lengths_of_class(g, 3)), ("np.sum", g, d)
    # the tree far-first (distance G / 2 first)
    d = _differs(t, lambda v: cr.lane_sum(v, far_first=True))
    for g in CLASSES:
        assert any(d[ln] for ln in _lengths_of_class(g, 3)), ("far-first", g, d)
    # the neighbouring class's lanes.  16 lanes on a longer column chain entries l and l + 16; 64
    # lanes on a column of <= 16 entries only add zeros (the same bits: that mistake cannot show,
    # and costs nothing), and so do 256 lanes up to 64 entries
    d = _differs(t, lambda v: cr.lane_sum(v, lanes=16))
    assert d[17] and all(d[ln] for ln in (63, 64, 65, 130, 4095, 4096)), ("16 lanes", d)
    assert not any(_differs(t, lambda v: cr.lane_sum(v, lanes=64))[ln] for ln in _lengths_of_class(16))
    d = _differs(t, lambda v: cr.lane_sum(v, lanes=256))
    assert not any(d[ln] for ln in (17, 63, 64)) and all(d[ln] for ln in (65, 130, 4095, 4096)), ("256 lanes", d)
    d = _differs(t, lambda v: cr.lane_sum(v, lanes=64))
    assert all(d[ln] for ln in _lengths_of_class(256)), ("64 lanes", d)  # 4097 among them
    # the block's waves in reverse order
    d = _differs(t, lambda v: cr.lane_sum(v, wave_order=(3, 2, 1, 0)))
    assert all(d[ln] for ln in _lengths_of_class(256)), ("waves reversed", d)
    assert not any(d[ln] for ln in cr.LENGTHS if ln <= 4096)


def test_fma_mutant_differs():
    """a contracted v * v + acc: the 16-lane class is exempt (its lanes add one product to 0, so
    contraction cannot show), and so is a wave's column of <= 64 entries"""
    t = cr.inexact_case("uniform")
    seen = {}
    for ln, v, _ in _cols(t):
        if ln in (16, 64, 130, 4096, 4097):
            seen[ln] = seen.get(ln, 0) + int(_bits([cr.ordered_sumsq(v)])[0] != _bits([_fma_sumsq(v)])[0])
    print("of 16 columns per length, sumsq differs under fma in:", seen)
    assert seen[16] == 0 and seen[64] == 0
    assert seen[130] and seen[4096] and seen[4097]


@pytest.mark.parametrize("pattern", ["uniform", "normal"])
def test_split_columns_differ_from_whole_ones(pattern):
    """the multi-rank test's matrix: summed block by block the bits differ from the 1 x 1 sum
    for some column, and for three ranks and more from the ranks in reverse order.  Two ranks
    cannot show their order: a + b = b + a by bits."""
    t = cr.split_case(pattern)
    half = t["m"] // 2
    lens = np.diff(t["cp"])
    upper = np.array([int(np.sum(r < half)) for _, _, r in _cols(t)])
    assert set(zip(upper.tolist(), (lens - upper).tolist())) == set(cr.SPLITS) and t["m"] <= 16500
    for what in ("sum", "sumsq"):
        whole, split = cr.reduce_cols_ordered(t, what), cr.reduce_cols_ordered(t, what, cuts=[half])
        diff = _bits(whole) != _bits(split)
        assert diff.any() and not diff[t["jc"][(upper == 0) | (upper == lens)]].any(), what
        print("%s: %d of %d split columns differ from the whole column's bits" % (what, diff.sum(), len(lens)))
    a, _ = cr.inflate_ordered(dict(t, val=np.abs(t["val"])))
    b, _ = cr.inflate_ordered(dict(t, val=np.abs(t["val"])), cuts=[half])
    assert np.any(_bits(a["val"]) != _bits(b["val"]))
    cuts = [half // 2, half, half + half // 2]
    fwd = rev = 0
    for ln, v, r in _cols(t):
        parts = [cr.ordered_sum(v[s]) for s in cr.split_rows(r, cuts)]
        assert cr.combine_ranks(parts) == cr.col_moment(v, r, "sum", cuts)
        rev += _bits([cr.combine_ranks(parts)])[0] != _bits([cr.combine_ranks(parts[::-1])])[0]
        two = [cr.ordered_sum(v[s]) for s in cr.split_rows(r, [half])]
        fwd += _bits([cr.combine_ranks(two)])[0] != _bits([cr.combine_ranks(two[::-1])])[0]
    assert rev > 0 and fwd == 0
