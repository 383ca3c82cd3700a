"""Without a GPU: the generators and host restatements that tests/test_gpu_tile_ops.py
compares the device with, each against a brute-force dense computation at tiny sizes
(at most 40 x 40), and the conditions that keep those GPU tests from becoming vacuous."""
import numpy as np

import helpers as H
import tile_ops_ref as R
from helpers import assert_tiles_bits_equal


def _tiny(seed, m=37, n=29, nnz=160):
    return R.random_tile(np.random.default_rng(seed), m, n, nnz)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_dense_round_trip_and_generators():
    for seed, (m, n, nnz) in enumerate([(37, 29, 160), (1, 40, 40), (40, 1, 17), (23, 19, 30), (5, 7, 0)]):
        d = R.random_tile(np.random.default_rng(seed), m, n, nnz)
        assert len(d["ir"]) == min(nnz, m * n) and H.digest(d)["unsorted"] == 0 and R.unsorted_host(d) == 0
        assert len(np.unique(d["val"])) == len(d["val"])
        assert_tiles_bits_equal(R.from_dense(*R.to_dense(d)), d)
    d = R.random_tile(np.random.default_rng(9), R.HUGE, R.HUGE, 50, corners=True)
    assert d["ir"].max() == R.HUGE - 1 and d["jc"].max() == R.HUGE - 1 and R.unsorted_host(d) == 0
    lens = [1, 5, 40, 3]
    d = R.cols_tile(np.random.default_rng(1), 40, 30, lens)
    assert sorted(np.diff(d["cp"]).tolist()) == sorted(lens) and R.unsorted_host(d) == 0
    d = R.regular_tile(np.random.default_rng(2), 40, 7, 200)
    assert len(d["ir"]) == 200 and R.unsorted_host(d) == 0 and sorted(d["val"].tolist()) == list(range(1, 201))
    R.to_dense(d)  # no position twice
    d = R.single_entry_cols_tile(np.random.default_rng(3), 30, 40, 25)
    assert np.all(np.diff(d["cp"]) == 1) and len(d["jc"]) == 25 and R.unsorted_host(d) == 0
    assert R.unsorted_host(R.one_row_tile(np.random.default_rng(4), 40, 40, 7, 30)) == 0
    assert R.unsorted_host(R.one_col_tile(np.random.default_rng(4), 40, 40, 7, 30)) == 0
    for d in (R.split_case(), R.single_col_case(), R.block_case(), R.digest_base()):
        assert R.unsorted_host(d) == 0 and H.digest(d)["unsorted"] == 0
    d = R.split_case()
    assert sorted(np.diff(d["cp"]).tolist()) == sorted(R.SPLIT_LENS * 2) and len(np.setdiff1d(np.arange(d["n"]), d["jc"]))
    assert 0 < d["ir"].min() and d["ir"].max() + 1 < d["m"]
    for nzc in R.REBUILD_SLOTS:
        d = R.rebuild_case(nzc)
        lens = np.diff(d["cp"])
        assert len(d["jc"]) == nzc and R.unsorted_host(d) == 0 and len(d["ir"]) < 4000
        assert nzc < 7 or set(R.SPLIT_LENS) <= set(lens.tolist())
        assert lens[0] == 1 and d["ir"][0] < 200 and (nzc == 1 or (lens[-1] == 65 and d["ir"][d["cp"][-2]] >= 400))
        assert nzc < 3 or (200 <= d["ir"][1:d["cp"][-2]].min() and d["ir"][1:d["cp"][-2]].max() < 400)
        top, bot = H.split_rows_host(d, 200)
        assert len(top["jc"]) == 1 and len(bot["jc"]) == nzc - 1
        assert len(np.setdiff1d(np.arange(int(d["jc"][0]) + 1, d["n"]), d["jc"]))  # a gap above the first id


def test_transpose_host_against_dense():
    for seed in range(4):
        d = _tiny(seed)
        held, vals = R.to_dense(d)
        assert_tiles_bits_equal(H.transpose_host(d), R.from_dense(held.T, vals.T))
    assert_tiles_bits_equal(H.transpose_host(R.empty_tile(3, 4)), R.empty_tile(4, 3))


def test_splits_concat_and_sub_tile_against_dense(cbg):
    d = _tiny(11)
    held, vals = R.to_dense(d)
    m, n = d["m"], d["n"]
    for cut in (0, n, int(d["jc"][3]), int(d["jc"][3]) + 1, 14):
        left, right = H.split_cols_host(d, cut)
        assert_tiles_bits_equal(left, R.from_dense(held[:, :cut], vals[:, :cut]))
        assert_tiles_bits_equal(right, R.from_dense(held[:, cut:], vals[:, cut:]))
        assert_tiles_bits_equal(H.concat_cols_host([left, right]), d)
    for cut in (0, m, 1, 18, m - 1):
        top, bot = H.split_rows_host(d, cut)
        assert_tiles_bits_equal(top, R.from_dense(held[:cut], vals[:cut]))
        assert_tiles_bits_equal(bot, R.from_dense(held[cut:], vals[cut:]))
    e = _tiny(12, n=11, nnz=50)
    he, ve = R.to_dense(e)
    z = R.empty_tile(m, 4)
    hz, vz = R.to_dense(z)
    assert_tiles_bits_equal(H.concat_cols_host([z, d, z, e, z]),
                            R.from_dense(np.hstack([hz, held, hz, he, hz]), np.hstack([vz, vals, vz, ve, vz])))
    assert_tiles_bits_equal(H.concat_cols_host([d]), d)
    for r0, r1, c0, c1 in ((0, m, 0, n), (0, 0, 0, n), (5, 5, 2, 9), (3, 4, 0, n), (0, m, 7, 8), (6, 30, 4, 29),
                           (0, m, n, n)):
        assert_tiles_bits_equal(cbg.sub_tile(d, r0, r1, c0, c1), R.from_dense(held[r0:r1, c0:c1], vals[r0:r1, c0:c1]))


def _ref_min(x, y):
    return x if x < y else y   # Operations.h:153-165


def _ref_max(x, y):
    return y if x < y else x   # Operations.h:167-179


def test_dim_apply_restatement_and_palette():
    """the min / max restatement against the reference's comparisons, scalar by scalar; the
    palette case holds every ordered (value, scaler) pair under Row and under Column"""
    P = R.PALETTE
    assert len(set(_bits(P).tolist())) == len(P) == 9
    d, vc, vr = R.dim_apply_case()
    assert sorted(set(np.diff(d["cp"]).tolist())) == sorted(R.DIM_LENS)
    assert len(vc) == d["n"] and len(vr) == d["m"] and R.unsorted_host(d) == 0
    want_pairs = {(a, b) for a in _bits(P).tolist() for b in _bits(P).tolist()}
    for dim, vec in ((R.COLUMN, vc), (R.ROW, vr)):
        assert R.palette_pairs(d, dim, vec) == want_pairs
        s = R.dim_scalers(d, dim, vec)
        for op, f in (("min", _ref_min), ("max", _ref_max), ("multiplies", lambda x, y: x * y),
                      ("plus", lambda x, y: x + y)):
            got = R.dim_apply_host(d, dim, vec, op)["val"]
            with np.errstate(all="ignore"):
                want = np.array([f(np.float64(x), np.float64(y)) for x, y in zip(d["val"], s)])
            if op in ("min", "max"):
                np.testing.assert_array_equal(_bits(got), _bits(want))   # an input handed through, NaN payload too
            else:
                assert np.array_equal(np.isnan(got), np.isnan(want))
                ok = ~np.isnan(want)
                np.testing.assert_array_equal(_bits(got[ok]), _bits(want[ok]))
    # the pairs on which fmin / fmax differ from the reference operators are present
    t = dict(d, val=np.array([1.5, np.nan, 0.0, -0.0]))
    t["cp"], t["jc"], t["ir"] = np.array([0, 4]), np.array([0], np.int32), np.arange(4, dtype=np.int32)
    s = np.array([np.nan, 1.5, -0.0, 0.0])
    lo, hi = R.dim_apply_host(t, R.ROW, s, "min")["val"], R.dim_apply_host(t, R.ROW, s, "max")["val"]
    assert np.isnan(lo[0]) and lo[1] == 1.5 and np.signbit(lo[2]) and not np.signbit(lo[3])
    assert hi[0] == 1.5 and np.isnan(hi[1]) and not np.signbit(hi[2]) and np.signbit(hi[3])
    assert np.fmin(t["val"], s)[0] == 1.5 and np.fmax(t["val"], s)[1] == 1.5


def test_merge_host_against_dense():
    """merge_host on tiny parts of every kind against a dense fold in part order"""
    for sr in ("plus", "minplus"):
        for P in (1, 2, 5, 9):
            rng = np.random.default_rng(40 + P)
            parts = []
            for p in range(P):
                nnz = 0 if p % 4 == 2 else int(rng.integers(1, 300))
                t = R.random_tile(rng, 33, 21, nnz)
                if sr == "plus":
                    t["val"] = rng.integers(-64, 64, len(t["ir"])).astype(np.float64) / 16.0
                parts.append(t)
            held = np.zeros((33, 21), bool)
            acc = np.zeros((33, 21))
            for t in parts:
                h, v = R.to_dense(t)
                new = h & ~held
                both = h & held
                acc[new] = v[new]
                acc[both] = acc[both] + v[both] if sr == "plus" else np.where(v[both] < acc[both], v[both], acc[both])
                held |= h
            assert_tiles_bits_equal(R.merge_host(parts, sr), R.from_dense(held, acc))


def test_merge_parts_cover_the_kinds():
    for sr in ("plus", "minplus"):
        for P in (1, 2, 5, 9):
            parts = R.merge_parts(P, sr)
            assert len(parts) == P and all((p["m"], p["n"]) == (parts[0]["m"], parts[0]["n"]) for p in parts)
            assert all(R.unsorted_host(p) == 0 for p in parts)
            want = R.merge_host(parts, sr)
            assert R.unsorted_host(want) == 0 and not np.isnan(want["val"]).any()
            keys = [set((H.tile_cols(p) * p["m"] + p["ir"]).tolist()) for p in parts]
            if P >= 2:
                assert set(parts[1]["jc"].tolist()) == set(parts[0]["jc"].tolist())      # the same columns,
                assert keys[1] & keys[0] and keys[1] - keys[0] and keys[0] - keys[1]     # some rows shared
            if P >= 5:
                assert not keys[2]                                         # an empty part
                assert not set(parts[3]["jc"].tolist()) & set(parts[0]["jc"].tolist())   # disjoint columns
                assert keys[4] == keys[0]                                  # overlap in every entry
            v = np.concatenate([p["val"] for p in parts])
            zeros = (v == 0.0)
            assert (zeros & np.signbit(v)).any() and (zeros & ~np.signbit(v)).any()
            if sr == "minplus":
                assert np.isinf(v).any() and (v == H.DBL_MAX).any() and (v == -H.DBL_MAX).any()
                # where parts meet: no zero, no tie between finite values (the minimum is order-free)
                allk = np.concatenate([H.tile_cols(p) * p["m"] + p["ir"] for p in parts])
                u, inv, cnt = np.unique(allk, return_inverse=True, return_counts=True)
                shared = v[cnt[inv] > 1]
                fin = shared[np.isfinite(shared)]
                assert not (shared == 0.0).any() and len(np.unique(fin)) == len(fin)


def test_digest_variants_match_the_documented_count():
    """the counts the GPU test asserts are the ones include/cbg.h's definition gives, and the
    malformed tiles stay inside their allocations"""
    names = set()
    for name, t, count in R.digest_variants():
        names.add(name)
        assert R.unsorted_host(t) == count, name
        nnz = len(t["ir"])
        assert np.all(np.diff(t["cp"]) >= 0) and 0 <= t["cp"][0] and t["cp"][-1] <= nnz
        assert 0 <= t["ir"].min() and t["ir"].max() < t["m"] and 0 <= t["jc"].min() and t["jc"].max() < t["n"]
    assert {"valid", "rows_swapped", "rows_equal", "rows_swapped_64_65", "jc_swapped", "jc_equal", "empty_column",
            "cp0_is_1", "cp_end_short", "two_violations"} <= names
    b = R.digest_base()
    assert len(b["jc"]) == 6 and np.diff(b["cp"]).max() > 64
    assert float(np.sum(b["val"])) == float(np.sum(b["val"][::-1]))
    # helpers.digest counts what it can see of the same definition
    assert H.digest(b)["unsorted"] == 0


def test_equal_cases_differ_in_one_entry():
    for base, others in R.equal_cases():
        for label, o in others:
            assert (o["m"], o["n"], len(o["ir"]), len(o["jc"])) == (base["m"], base["n"], len(base["ir"]), len(base["jc"]))
            diff = sum(int(np.sum(np.asarray(o[k]) != np.asarray(base[k]))) for k in ("cp", "jc", "ir", "val"))
            assert diff == 1, label
            assert np.all(np.diff(o["cp"]) >= 0) and o["cp"][-1] <= len(o["ir"])
            if label != "cp[nzc]":
                assert R.unsorted_host(o) == 0, label
    (_, _), (one, _) = R.equal_cases()
    assert len(one["ir"]) == len(one["jc"]) < len(one["jc"]) + 1


def test_restriction_input_is_strong_enough():
    """scale 13: 8157 draws (two sort tiles), at least 500 rows with 3 or more draws, and
    with order = 8192 every such row is one run of equal keys"""
    draws = R.restriction_row_draws(13)
    assert int(draws.sum()) == 8157 and R.SORT_TILE < 8157 <= 2 * R.SORT_TILE
    assert int((draws >= 3).sum()) >= 500
    for order, kept in ((2, 8156), (4096, 6417), (8192, 5148)):
        g = H.restriction_host(13, order)
        assert len(g["ir"]) == kept and g["n"] == (1 << 13) // order and R.unsorted_host(g) == 0
    g = H.restriction_host(13, 8192)
    assert len(g["jc"]) == 1 and len(g["ir"]) == int((draws > 0).sum())


def test_pass_table_covers_one_to_eight():
    """low_bits' rule restated: the shapes of the transpose test make 1 to 8 digit passes"""
    assert R.low_bits(0) == 0 and R.low_bits(1) == 1 and R.low_bits(255) == 255 and R.low_bits(256) == 511
    assert R.low_bits(69999) == (1 << 17) - 1 and R.low_bits(R.HUGE - 1) == (1 << 31) - 1
    got = [R.transpose_passes(m, n) for (m, n), _ in R.PASS_SHAPES]
    assert got == [p for _, p in R.PASS_SHAPES]
    assert set(got) == set(range(1, 9))
    assert R.transpose_passes(*R.NNZ_EDGE_SHAPE) == 5          # 2 + 3: odd
    assert R.transpose_passes(1024, 1024) == 4                 # the one shape tested before: even
    assert R.digit_passes(1, 8192) == 2 and R.digit_passes(2, 4096) == 3   # restriction, order 8192 / 4096
    assert R.HUGE < np.iinfo(np.int32).max
    edges = set(R.NNZ_EDGES)
    for b in (64, 256, R.SORT_TILE, 2 * R.SORT_TILE):
        assert {b - 1, b, b + 1} <= edges
