"""The restatement of the matrix x vector products (tests/spmv_ref.py) against the reference's own
outputs in tests/golden/spmv_*.npz (made by tests/golden/make_spmv_golden.py): CPU only."""
import numpy as np
import pytest

import colsum_ref as cr
import spmv_ref as sv
from spmv_worker import CASES, SEMIRINGS, SPARSE, load_case, split_case


def same_bits(a, b):
    return np.array_equal(sv.bits(a), sv.bits(b))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("s,sr", SEMIRINGS)
def test_restatement_agrees_with_the_reference(name, s, sr):
    """bit-equal for MinPlus and the exact sums; PlusTimes on inexact values within the bound of two
    orderings of the same rounded products, every row checked"""
    z, ts = load_case(name)
    t, x = ts[s], z["x_" + s]
    exact = name == "dyadic" or sr == sv.MIN_PLUS
    for cuts, pc in ((None, 1), ([t["n"] // 2], 2)):
        y = sv.spmv(t, x, sr, cuts)
        for ref in (z["y_" + s], z["y4_" + s]):
            if exact:
                assert same_bits(y, ref)
            else:
                assert np.all(np.abs(y - ref) <= sv.bound(t, x, pc=2))
        empty = sv.row_lengths(t) == 0
        assert np.all(y[empty] == sv.ID[sr]) and (name == "rect" or empty.sum() == 453)
        for k in SPARSE:
            ids = z["xs_" + k]
            yi, yv = sv.spmspv(t, ids, x[ids], sr, cuts)
            for pre in ("ys", "ys4"):
                ri, rv = z[f"{pre}_{s}_{k}_ind"], z[f"{pre}_{s}_{k}_val"]
                assert np.array_equal(yi, ri)
                if exact:
                    assert same_bits(yv, rv)
                else:
                    # L and the sum run over the products of the columns that take part
                    sub = sv.restrict_cols(t, ids)
                    assert np.all(np.abs(yv - rv) <= sv.bound(sub, x, pc=2)[yi])


def test_the_order_matters_on_inexact_values():
    z, ts = load_case("rmat")
    t, x = ts["pt"], z["x_pt"]
    y = sv.spmv(t, x)
    other = sv.spmv(t, x, lanes=32)
    assert not same_bits(y, other)
    assert np.all(np.abs(y - other) <= sv.bound(t, x))
    # a column cut changes the order too
    assert not same_bits(y, sv.spmv(t, x, cuts=[512]))
    # MinPlus is order-free
    assert same_bits(sv.spmv(ts["mp"], z["x_mp"], sv.MIN_PLUS), sv.spmv(ts["mp"], z["x_mp"], sv.MIN_PLUS, lanes=32))


def test_the_dyadic_case_is_order_free():
    z, ts = load_case("dyadic")
    for s, sr in SEMIRINGS:
        t, x = ts[s], z["x_" + s]
        y = sv.spmv(t, x, sr)
        assert same_bits(y, z["y_" + s]) and same_bits(y, z["y4_" + s])
        for lanes, cuts in ((32, None), (4, [100, 700]), (None, [512])):
            assert same_bits(y, sv.spmv(t, x, sr, cuts, lanes))
        ids = z["xs_even"]
        yi, yv = sv.spmspv(t, ids, x[ids], sr)
        oi, ov = sv.spmspv(t, ids, x[ids], sr, [300], 8)
        assert np.array_equal(yi, oi) and same_bits(yv, ov)


def test_lane_fold_written_out():
    """lanes_reduce against a lane-by-lane fold from the device's identities, the -0.0 start included"""
    rng = np.random.default_rng(5)

    def direct(p, sr, g):
        ident = -0.0 if sr == sv.PLUS_TIMES else np.inf
        acc = [ident] * g
        for k, v in enumerate(p.tolist()):
            acc[k % g] = sv.add(sr, acc[k % g], v)
        d = 1
        while d < g:
            acc = [sv.add(sr, acc[i], acc[i ^ d]) for i in range(g)]
            d *= 2
        return acc[0]

    for sr in (sv.PLUS_TIMES, sv.MIN_PLUS):
        for n in (1, 2, 15, 16, 17, 63, 64, 65, 200, 4096):
            p = cr.pattern_values(rng, "normal", n)
            g = 16 if n <= 16 else 64
            assert same_bits(sv.row_reduce(p, sr), direct(p, sr, g))
        for p in (np.full(3, -0.0), np.array([-0.0, 0.0]), np.array([1.5, -1.5]), np.full(20, -0.0)):
            assert same_bits(sv.row_reduce(p, sr), direct(p, sr, 16 if len(p) <= 16 else 64))
    assert np.signbit(sv.row_reduce(np.full(3, -0.0), sv.PLUS_TIMES))
    assert not np.signbit(sv.fold_id(sv.PLUS_TIMES, -0.0))


def test_chunks_and_sentinels():
    rng = np.random.default_rng(6)
    p = cr.pattern_values(rng, "wide", 2 * 4096 + 1)
    parts = [sv.lanes_reduce(p[c:c + 4096], sv.PLUS_TIMES, 64) for c in (0, 4096, 8192)]
    assert same_bits(sv.row_reduce(p, sv.PLUS_TIMES), (parts[0] + parts[1]) + parts[2])
    assert same_bits(sv.lanes_reduce(p[8192:], sv.PLUS_TIMES, 64), p[8192])
    # inf_plus and the dense fold with DBL_MAX
    assert sv.mul(sv.MIN_PLUS, sv.DBL_MAX, -5.0) == sv.DBL_MAX and sv.mul(sv.MIN_PLUS, 1.0, sv.DBL_MAX) == sv.DBL_MAX
    assert sv.fold_id(sv.MIN_PLUS, np.inf) == sv.DBL_MAX and sv.fold_id(sv.MIN_PLUS, 3.0) == 3.0
    t, x = split_case()
    lens = sv.row_lengths(t)
    assert sorted(set(lens.tolist())) == [0, 30, 33, 8193]
