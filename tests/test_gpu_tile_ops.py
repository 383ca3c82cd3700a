"""The code under every SUMMA stage, phase, Galerkin product and R-MAT tile, at its edges:
the LSD radix sort and reduce-by-key (csrc/cbg_sort.hip), the multi-level scan
(csrc/cbg_tile.hip) and the structural tile operations (cbg_tile.hip, cbg_ops.hip).

Every comparison is against a NumPy restatement on the host (tests/helpers.py,
tests/tile_ops_ref.py; tests/test_tile_ops_cpu.py checks those against dense brute
force) and is by bits; every device result must digest with unsorted == 0.
"""
import numpy as np
import pytest

import tile_ops_ref as R
from helpers import (assert_tiles_bits_equal, concat_cols_host, digest, restriction_host, split_cols_host,
                     split_rows_host, transpose_host)

pytestmark = pytest.mark.gpu


def _self_grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def _check(tile, want, nan_payload=False):
    """device tile == host tile by bits, and a valid DCSC tile"""
    got = tile.to_host()
    assert_tiles_bits_equal(got, want)
    if nan_payload:  # the values are copies of inputs: a NaN keeps its sign and payload too
        np.testing.assert_array_equal(np.ascontiguousarray(got["val"]).view(np.uint64),
                                      np.ascontiguousarray(want["val"], dtype=np.float64).view(np.uint64))
    d = tile.digest()
    assert d["unsorted"] == 0 and d["nnz"] == len(want["ir"]) and d["nzc"] == len(want["jc"])
    return got


def _check_transpose(cbg, d):
    t = cbg.Tile.from_dict(d)
    tt = t.transpose()
    _check(tt, transpose_host(d))
    _check(tt.transpose(), d)
    return tt


# --------------------------------------------------------------------------
# a. transpose across the sort's edges
# --------------------------------------------------------------------------
def _transpose_cases():
    cases = []
    for i, nnz in enumerate(R.NNZ_EDGES):
        cases.append(pytest.param(lambda i=i, nnz=nnz: R.random_tile(np.random.default_rng(100 + i), *R.NNZ_EDGE_SHAPE, nnz),
                                  id=f"nnz{nnz}"))
    for i, ((m, n), passes) in enumerate(R.PASS_SHAPES):
        cases.append(pytest.param(
            lambda i=i, m=m, n=n: R.random_tile(np.random.default_rng(200 + i), m, n, R.PASS_NNZ, corners=m > 1 << 20),
            id=f"passes{passes}_{m}x{n}"))
    # the row (column) digits are in the mask but constant over the keys
    cases.append(pytest.param(lambda: R.one_row_tile(np.random.default_rng(301), 70000, 70000, 66051, 5000), id="one_row"))
    cases.append(pytest.param(lambda: R.one_col_tile(np.random.default_rng(302), 70000, 70000, 66051, 5000), id="one_col"))
    cases.append(pytest.param(
        lambda: R.cols_tile(np.random.default_rng(303), 3000, 500,
                            np.random.default_rng(304).choice([1, 63, 64, 65, 130], 120)), id="col_lens"))
    cases.append(pytest.param(lambda: R.empty_tile(300, 70000), id="empty"))
    return cases


@pytest.mark.parametrize("make", _transpose_cases())
def test_transpose_sort_edges(cbg, make):
    """Tile.transpose against transpose_host (np.lexsort): nnz around the wave (64), the
    block (256) and one and two sort tiles (4096, 8192); 1 to 8 digit passes, odd counts
    included (the ping-pong buffers); digits in the mask that no key varies in; row ids of
    four digits; partial last waves and tiles; and transpose(transpose(t)) == t."""
    d = make()
    _check_transpose(cbg, d)


# --------------------------------------------------------------------------
# b. the scan's levels
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nzc", [R.SCAN_TILE - 1, R.SCAN_TILE, R.SCAN_TILE + 1])
def test_scan_tile_boundary(cbg, nzc):
    """single-entry columns with gaps, nzc = nnz = 2048 - 1, 2048, 2048 + 1: keys_to_tile's
    scan over nnz flags and split_rows' four scans over nzc at the one-level / two-level edge"""
    d = R.single_entry_cols_tile(np.random.default_rng(400 + nzc), 2500, 3000, nzc)
    _check_transpose(cbg, d)
    t = cbg.Tile.from_dict(d)
    for cut in (1250, 1):
        top, bot = t.split_rows(cut)
        wt, wb = split_rows_host(d, cut)
        _check(top, wt)
        _check(bot, wb)


@pytest.mark.parametrize("nnz", [R.SCAN_TILE ** 2 + 3, R.SCAN_TILE ** 2 - 1])
def test_scan_third_level(cbg, nnz):
    """nnz = 2048^2 + 3 (three scan levels inside keys_to_tile) and 2048^2 - 1 (two full ones)"""
    d = R.regular_tile(np.random.default_rng(500), 3001, 1500, nnz)
    _check_transpose(cbg, d)


# --------------------------------------------------------------------------
# c. stability of the multi-tile sort and reduce-by-key
# --------------------------------------------------------------------------
_RESTRICT = {}


def _restriction(order):
    if order not in _RESTRICT:
        _RESTRICT[order] = restriction_host(13, order)
    return _RESTRICT[order]


@pytest.mark.parametrize("order,kept", [(2, 8156), (4096, 6417), (8192, 5148)])
def test_restriction_sort_stability(cbg, order, kept):
    """restriction_tile(13, order) bit for bit: 8157 drawn entries (two sort tiles); with
    order = 8192 there is one coarse column, so every fine row that drew k entries is a
    run of k equal keys, whose sum depends on the order when k >= 3: only a stable sort
    and an in-order reduce-by-key give the host's bits.  1 x 1, and every tile of a 2 x 3
    grid against its block of the global operator."""
    draws = R.restriction_row_draws(13)
    assert int(draws.sum()) == 8157 > R.SORT_TILE
    assert int((draws >= 3).sum()) >= 500
    g = _restriction(order)
    assert len(g["ir"]) == kept
    _check(cbg.restriction_tile(13, order), g)
    for prow in range(2):
        for pcol in range(3):
            r0, r1 = cbg.block_range(g["m"], 2, prow)
            c0, c1 = cbg.block_range(g["n"], 3, pcol)
            _check(cbg.restriction_tile(13, order, grid=(2, 3), pos=(prow, pcol)), cbg.sub_tile(g, r0, r1, c0, c1))


# --------------------------------------------------------------------------
# d. dim_apply
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dim", ["Column", "Row"])
@pytest.mark.parametrize("op", ["multiplies", "plus", "min", "max"])
def test_dim_apply_palette(cbg, op, dim):
    """op(value, scaler) over every ordered pair of {+-0.0, +-1.5, +-inf, NaN, 5e-324,
    DBL_MAX}, in columns of 1, 64, 65 and 200 entries.  min and max are the reference's
    minimum(x, y) = x < y ? x : y and maximum(x, y) = x < y ? y : x (Operations.h:153-179),
    not fmin / fmax: whenever the comparison is false -- a NaN on either side, +0.0 against
    -0.0 -- min returns the scaler and max the value; all 64 bits are compared (min and
    max hand one of their inputs through).  multiplies and plus: NaN where the reference has
    NaN, every other value by bits."""
    d, vc, vr = R.dim_apply_case()
    dimc, vec = (cbg.Column, vc) if dim == "Column" else (cbg.Row, vr)
    assert len(R.palette_pairs(d, dimc, vec)) == len(R.PALETTE) ** 2
    t = cbg.Tile.from_dict(d)
    t.dim_apply(dimc, vec, op)
    want = R.dim_apply_host(d, dimc, vec, op)
    got = t.to_host()
    if op in ("min", "max"):
        v, s = d["val"], R.dim_scalers(d, dimc, vec)
        gb, wb = got["val"].view(np.uint64), np.ascontiguousarray(want["val"]).view(np.uint64)
        bad = np.flatnonzero(gb != wb)
        first = [(float(v[i]), float(s[i]), float(got["val"][i]), float(want["val"][i])) for i in bad[:8]]
        print(f"{op} {dim}: {len(bad)} of {len(wb)} differ; first (value, scaler, got, want): {first}")
        assert len(bad) == 0, f"{len(bad)} of {len(wb)} differ; first (value, scaler, got, want): {first}"
    _check(t, want, nan_payload=op in ("min", "max"))


def test_dim_apply_empty_and_wrong_length(cbg):
    z = cbg.Tile.from_dict(R.empty_tile(4, 3))
    for dimc, k in ((cbg.Column, 3), (cbg.Row, 4)):
        for op in ("multiplies", "plus", "min", "max"):
            z.dim_apply(dimc, np.full(k, np.nan), op)
    _check(z, R.empty_tile(4, 3))
    d, vc, vr = R.dim_apply_case()
    t = cbg.Tile.from_dict(d)
    for dimc, vec in ((cbg.Column, vr), (cbg.Row, vc), (cbg.Column, vc[:-1]), (cbg.Row, np.zeros(0))):
        with pytest.raises(cbg.CbgError) as e:
            t.dim_apply(dimc, vec, "min")
        assert e.value.code == cbg.INVALIDPARAMS
    _check(t, d, nan_payload=True)   # untouched


# --------------------------------------------------------------------------
# e. the digest's unsorted count
# --------------------------------------------------------------------------
def test_digest_counts_order_violations(cbg):
    """Tile.digest()["unsorted"] is what nearly every GPU test trusts as its "valid DCSC"
    check: it must count each violation that include/cbg.h documents, exactly"""
    for name, t, count in R.digest_variants():
        got = cbg.Tile.from_dict(t).digest()
        assert got["unsorted"] == count, (name, got, count)
    b = R.digest_base()
    got, want = cbg.Tile.from_dict(b).digest(), digest(b)
    assert want["unsorted"] == 0
    assert (got["nnz"], got["nzc"], got["hs"], got["hv"], got["vsum"]) == \
        (want["nnz"], want["nzc"], want["hs"], want["hv"], want["vsum"])
    got, want = cbg.Tile.from_dict(b).digest(1000, 77), digest(b, 1000, 77)
    assert (got["hs"], got["hv"]) == (want["hs"], want["hv"])


# --------------------------------------------------------------------------
# f. tile_equal on structure
# --------------------------------------------------------------------------
def test_tile_equal_structure(cbg):
    """equal m, n, nnz and nzc; one jc or one interior cp entry differs (the first, a middle
    one, the last): not equal.  Every tile is a valid one, but for the single-entry-column
    pair that differs in cp[nzc] alone -- index nzc is beyond nnz there, the kernel's loop
    bound is max(nnz, nzc + 1), and k_tile_diff reads the arrays element by element only."""
    for base, others in R.equal_cases():
        A = cbg.Tile.from_dict(base)
        assert A == cbg.Tile.from_dict(base)
        assert A == cbg.Tile.from_dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()})
        for label, other in others:
            B = cbg.Tile.from_dict(other)
            assert (A.m, A.n, A.nnz, A.nzc) == (B.m, B.n, B.nnz, B.nzc)
            assert not A == B, label
            assert not B == A, label


# --------------------------------------------------------------------------
# g. splits, concatenation and slices
# --------------------------------------------------------------------------
def _split_tiles():
    """the last five: the column-rebuild primitive's slot counts (tile_ops_ref.rebuild_case)"""
    return [("gaps", R.split_case()), ("single_col", R.single_col_case())] + [
        (f"slots{k}", R.rebuild_case(k)) for k in R.REBUILD_SLOTS]


def _col_cuts(d):
    stored = int(d["jc"][len(d["jc"]) // 2])
    gap = int(np.setdiff1d(np.arange(int(d["jc"][0]) + 1, d["n"]), d["jc"])[0])
    last_before_gap = int(d["jc"][-1])
    return sorted({0, d["n"], stored, stored + 1, int(d["jc"][0]), last_before_gap, last_before_gap + 1, gap})


def _row_cuts(d):
    lo, hi = int(d["ir"].min()), int(d["ir"].max())
    mid = int(np.sort(d["ir"])[len(d["ir"]) // 2])
    # just past the first column's last row, and the last column's first row: in a rebuild_case
    # these empty the first (the last) column alone on one side, every other one on the other
    past_first, at_last = int(d["ir"][d["cp"][1] - 1]) + 1, int(d["ir"][d["cp"][-2]])
    return sorted({0, d["m"], mid, mid + 1, hi + 1, hi, lo, lo + 1, past_first, at_last})


def test_split_cols_cuts(cbg):
    """cut 0, n, a stored column id, a stored id + 1, an id inside a gap"""
    for name, d in _split_tiles():
        t = cbg.Tile.from_dict(d)
        for cut in _col_cuts(d):
            left, right = t.split_cols(cut)
            wl, wr = split_cols_host(d, cut)
            _check(left, wl)
            _check(right, wr)
            _check(cbg.Tile.concat_cols([left, right]), d)
        _check(t, d)


def test_split_rows_cuts(cbg):
    """cut 0, m, a stored row, and cuts that send every entry to the top or to the bottom"""
    for name, d in _split_tiles():
        t = cbg.Tile.from_dict(d)
        for cut in _row_cuts(d):
            top, bot = t.split_rows(cut)
            wt, wb = split_rows_host(d, cut)
            assert len(wt["ir"]) + len(wb["ir"]) == len(d["ir"])
            _check(top, wt)
            _check(bot, wb)
        lo, hi = int(d["ir"].min()), int(d["ir"].max())
        assert 0 < lo and hi + 1 < d["m"]
        assert t.split_rows(hi + 1)[1].nnz == 0 and t.split_rows(lo)[0].nnz == 0
        _check(t, d)


def test_concat_cols_parts(cbg):
    """1 part; 5 parts with empty ones first, in the middle and last"""
    d, s = R.split_case(), R.single_col_case()
    _check(cbg.Tile.concat_cols([cbg.Tile.from_dict(d)]), concat_cols_host([d]))
    hosts = [R.empty_tile(d["m"], 3), d, R.empty_tile(d["m"], 5), s, R.empty_tile(d["m"], 1)]
    _check(cbg.Tile.concat_cols([cbg.Tile.from_dict(h) for h in hosts]), concat_cols_host(hosts))
    hosts = [R.empty_tile(d["m"], 2), R.empty_tile(d["m"], 0), R.empty_tile(d["m"], 4)]
    _check(cbg.Tile.concat_cols([cbg.Tile.from_dict(h) for h in hosts]), R.empty_tile(d["m"], 6))


@pytest.mark.parametrize("parts", [1, 2, 7, 40])
def test_colsplit_parts(cbg, parts):
    """ColSplit(parts): pieces cut at (i + 1) * (n // parts), the last taking the rest;
    parts = n gives single-column pieces; their concatenation is the input"""
    d = R.split_case()
    assert d["n"] == 40
    pieces = cbg.Tile.from_dict(d).ColSplit(parts)
    assert len(pieces) == parts
    w, rest, want = d["n"] // parts, d, []
    for i in range(parts - 1):
        left, rest = split_cols_host(rest, w)
        want.append(left)
    want.append(rest)
    for p, h in zip(pieces, want):
        _check(p, h)
    _check(cbg.Tile.concat_cols(pieces), d)


def test_block_extract_ranges(cbg):
    """SpParMat._block_extract on a 1 x 1 grid, both dims: [0, 0), [k, k), [0, size), one row,
    one column, a range whose ends fall in gaps, a range ending at size"""
    g = _self_grid(cbg)
    for name, d in _split_tiles():
        A = cbg.SpParMat.from_global(g, d)
        free_cols = np.setdiff1d(np.arange(d["n"]), d["jc"])
        free_rows = np.setdiff1d(np.arange(d["m"]), d["ir"])
        row, col = int(d["ir"][len(d["ir"]) // 2]), int(d["jc"][-1])
        for dim, size, one, ids, gaps in ((0, d["m"], row, d["ir"], free_rows), (1, d["n"], col, d["jc"], free_cols)):
            inner = gaps[(gaps > ids.min()) & (gaps < ids.max())]   # unused ids between stored ones
            inner = inner if len(inner) >= 2 else gaps
            ranges = [(0, 0), (size // 2, size // 2), (size, size), (0, size), (one, one + 1),
                      (int(inner[0]), int(inner[-1])), (size // 3, size), (int(gaps[0]), int(gaps[0]) + 1)]
            for lo, hi in ranges:
                B = A._block_extract(dim, lo, hi)
                want = cbg.sub_tile(d, lo, hi, 0, d["n"]) if dim == 0 else cbg.sub_tile(d, 0, d["m"], lo, hi)
                assert (B.gm, B.gn) == (want["m"], want["n"])
                _check(B.tile, want)
        _check(A.tile, d)
    g.destroy()


@pytest.mark.parametrize("br", [1, 5, 7])
@pytest.mark.parametrize("bc", [1, 5, 7])
def test_block_split_uneven(cbg, br, bc):
    """BlockSplit(br, bc) of a 23 x 19 tile: blocks of uneven size, some of them empty"""
    g = _self_grid(cbg)
    d = R.block_case()
    A = cbg.SpParMat.from_global(g, d)
    blocks = A.BlockSplit(br, bc)
    if br == 1 and bc == 1:
        assert blocks[0][0] is A
    roff, coff = cbg._block_offsets(d["m"], br), cbg._block_offsets(d["n"], bc)
    assert roff[-1] == d["m"] and coff[-1] == d["n"] and len(roff) == br + 1 and len(coff) == bc + 1
    empty = total = 0
    for i in range(br):
        for j in range(bc):
            want = cbg.sub_tile(d, roff[i], roff[i + 1], coff[j], coff[j + 1])
            _check(blocks[i][j].tile, want)
            empty += len(want["ir"]) == 0
            total += len(want["ir"])
    assert total == len(d["ir"])
    if br == 7 and bc == 7:
        assert empty > 0
    g.destroy()


# --------------------------------------------------------------------------
# h. merge with many parts
# --------------------------------------------------------------------------
@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("P", [1, 2, 5, 9])
def test_merge_many_parts(cbg, P, sr):
    """MergeAll of P host-built partials: empty parts, disjoint columns, parts that overlap
    in every entry or share only some rows of a column.  plus: dyadic values and both
    zeros (exact in any order); minplus: +-0.0, +inf and the DBL_MAX sentinels handed
    through at positions one part holds, distinct values where parts meet.  The reference
    is a host fold over (col, row) keys in part order."""
    parts = R.merge_parts(P, sr)
    want = R.merge_host(parts, sr)
    if P >= 5:
        assert any(len(p["ir"]) == 0 for p in parts)
        assert len(want["ir"]) < sum(len(p["ir"]) for p in parts)
    tiles = [cbg.Tile.from_dict(p) for p in parts]
    _check(cbg.MergeAll(tiles, sr), want)
    for t, p in zip(tiles, parts):
        _check(t, p)  # the inputs are untouched
