"""The operands of tests/test_gpu_aprep_cache.py are what they claim (no device): every
block kind of helpers.APREP_SEQUENCES against the thresholds the multiply's routes turn on,
from the oracle's flops per column (oracle_symbolic) -- the number of big and thin columns
under the cut the lower-cut rule picks, the big columns' B entries against A's stored
columns / the entries factor, their flops against the flops factor x nnz(A), B's
integrality, zeros and column sums against 2^31 / max |a| for both integer value sets --
and the oracle's C of every piece is non-empty and holds what its kind is there for."""
import numpy as np
import pytest

import helpers as H

NNZ_A, NZC_A, R = 328000, 4200, 5


def _blocks():
    for seq in sorted(H.APREP_SEQUENCES):
        Bh, kinds = H.aprep_B(seq)
        for p, (kind, Bp) in enumerate(zip(kinds, H.aprep_pieces(Bh, len(kinds)))):
            yield seq, p, kind, Bp


def test_a_value_sets():
    A = H.aprep_A("int")
    assert (A["m"], len(A["jc"]), len(A["ir"])) == ((1 << 20) + 77, NZC_A, NNZ_A)
    assert (A["m"] + H.PANEL - 1) // H.PANEL == R >= 4
    assert A["n"] == NZC_A + H.APREP_EMPTY_A and int(A["jc"][-1]) == NZC_A - 1    # the empty columns come last
    for values in H.APREP_A_VALUES:
        v = H.aprep_A(values)["val"]
        for k in ("cp", "jc", "ir"):
            np.testing.assert_array_equal(H.aprep_A(values)[k], A[k])               # one structure
        with np.errstate(over="ignore"):
            f32_exact = bool((v.astype(np.float32).astype(np.float64) == v).all())  # (NaN: none in A)
        integral = bool(((v == np.trunc(v)) & (v != 0) & (np.abs(v) <= 2.0 ** 24)).all())
        assert f32_exact == (values != "f64"), values
        assert integral == values.startswith("int"), values
    assert np.abs(H.aprep_A("int")["val"]).max() == 4.0
    big = H.aprep_A("int_big")["val"]
    assert big[0] == 2.0 ** 24 and (np.abs(big) == 2.0 ** 24).sum() == 1 and np.abs(big[1:]).max() == 4.0
    assert int(A["jc"][0]) == 0    # the 2^24 sits in A's column 0, where B_heavy puts its large value


def test_sequences_cover_the_kinds():
    used = {k for s in H.APREP_SEQUENCES.values() for k in s}
    assert used == set(H.APREP_KINDS)
    for seq in sorted(H.APREP_SEQUENCES):
        Bh, kinds = H.aprep_B(seq)
        assert Bh["n"] == H.APREP_W * len(kinds) and Bh["m"] == H.aprep_A("int")["n"]
        assert H.APREP_W % 256 == 0      # the plan's sample takes column 0 of every block
    # that sample of sequence (a) has enough big-column entries for the full panel map
    A, (Bh, kinds) = H.aprep_A("int"), H.aprep_B("a")
    f = H.oracle_symbolic(A, Bh)[0]
    pick = (Bh["jc"] % 256 == 0) & (f > H.BIG_FLOPS)
    assert pick.sum() >= 2 and int(np.diff(Bh["cp"])[pick].sum()) * H.APREP_ENTRIES >= NZC_A


@pytest.mark.parametrize("seq,p,kind", [(s, p, k) for s, p, k, _ in _blocks()])
def test_block_is_its_kind(seq, p, kind):
    A = H.aprep_A("int")
    Bp = H.aprep_pieces(H.aprep_B(seq)[0], len(H.APREP_SEQUENCES[seq]))[p]
    fa = H.aprep_piece_facts(A, Bp)
    few_entries = fa["big_entries"] * H.APREP_ENTRIES < NZC_A
    pays_rvd = fa["big_flops"] >= H.APREP_RVD_FLOPS * NNZ_A
    v = np.asarray(Bp["val"], np.float64)
    print(seq, p, kind, {k: x for k, x in fa.items() if not k.startswith("col_")})
    if kind == "empty":
        assert fa["stored"] == 0 and len(Bp["ir"]) == 0
        return
    assert fa["stored"] > 0
    # sums: every f64 sum stays an exact integer (below 2^53) with int_big's 2^24
    assert 2.0 ** 24 * fa["b_colsum"] < 2.0 ** 53
    if kind == "small":
        assert fa["nbig"] == 0 and fa["nthin"] == 0 and fa["cut"] == H.BIG_FLOPS
        assert fa["moved"] > 0 and not fa["low_cond"]         # columns the lower cut would move, no big ones: it stays out
    elif kind == "lean":
        assert fa["nbig"] in (1, 2) and fa["nthin"] == 0
        assert few_entries and not pays_rvd
        assert fa["moved"] > 0 and not fa["low_cond"] and fa["cut"] == H.BIG_FLOPS
    elif kind == "thin":
        assert fa["nthin"] >= 1 and fa["nbig"] >= 1 and fa["cut"] == H.BIG_FLOPS and fa["moved"] == 0
        assert few_entries and not pays_rvd
    else:
        assert kind in H.APREP_RICH_LIKE
        assert fa["nbig"] >= 100 and fa["nthin"] == 0
        assert not few_entries and pays_rvd
        assert fa["over_flops"] >= H.APREP_RVD_FLOPS * NNZ_A         # ... also without the columns the lower cut adds
        # the lower cut fires: columns between the cuts, and the ones above 4096 carry >= half of the flops
        assert fa["moved"] > 0 and fa["low_cond"] and 2 * fa["over_flops"] >= fa["flops"] and fa["cut"] == H.LOW_CUT_FLOPS
        # panel groups of 4 and of 2, and (column, panel) pairs on their own
        f = fa["col_flops"][fa["col_big"]]
        g4, g2 = H.GROUP_PRODUCTS * R // 4, H.GROUP_PRODUCTS * R // 2
        assert min((f <= g4).sum(), ((f > g4) & (f <= g2)).sum(), (f > g2).sum()) >= 10
    # B's values: nonzero integers but for the entry that names the kind
    odd = np.flatnonzero((v != np.trunc(v)) | (v == 0))
    if kind in ("B_half", "B_zero"):
        assert len(odd) == 1 and not fa["b_integral"]
        assert v[odd[0]] == (0.5 if kind == "B_half" else 0.0) and not np.signbit(v[odd[0]])
        col = int(np.searchsorted(Bp["cp"], odd[0], side="right")) - 1
        assert fa["col_big"][col] and int(Bp["ir"][odd[0]]) == 0       # in a big column, on A's column 0
    else:
        assert len(odd) == 0 and fa["b_integral"]
    # the int32 bound max|a| x (largest column sum of |b|) < 2^31 for both integer value sets
    if kind == "B_heavy":
        assert 4 * fa["b_colsum"] < 2.0 ** 31 <= 2.0 ** 24 * fa["b_colsum"]
        at = int(np.argmax(np.abs(v)))
        col = int(np.searchsorted(Bp["cp"], at, side="right")) - 1
        assert v[at] == H.APREP_HEAVY_B and fa["col_big"][col] and int(Bp["ir"][at]) == 0
    elif kind == "thin":
        assert 4 * fa["b_colsum"] < 2.0 ** 31 <= 2.0 ** 24 * fa["b_colsum"]     # (the thin columns' many entries)
    else:
        assert 2.0 ** 24 * fa["b_colsum"] < 2.0 ** 31


@pytest.mark.parametrize("seq", sorted(H.APREP_SEQUENCES))
@pytest.mark.parametrize("values,sr", [(v, sr) for v, srs in H.APREP_A_VALUES.items() for sr in srs])
def test_oracle_pieces_hold_what_the_kinds_are_for(seq, values, sr):
    kinds = H.APREP_SEQUENCES[seq]
    refs = H.aprep_refs(seq, values, sr)
    assert len(refs) == len(kinds)
    for kind, C in zip(kinds, refs):
        v = np.asarray(C["val"], np.float64)
        assert C["n"] == H.APREP_W and C["m"] == (1 << 20) + 77
        if kind == "empty":
            assert len(v) == 0
            continue
        assert len(v) > 0
        if values in ("f32", "f64"):
            H.assert_palette_not_vacuous(C, values)
            continue
        assert not np.isnan(v).any() and np.abs(v).max() < 2.0 ** 53
        if sr != "plus":
            continue
        negzero = int(((v == 0) & np.signbit(v)).sum())
        if kind == "B_half":      # int32 accumulation would truncate these
            assert (v != np.trunc(v)).any()
        elif kind == "B_zero":    # ... and lose these
            assert negzero >= 1
        else:
            assert (v == np.trunc(v)).all() and negzero == 0
        if kind == "B_heavy":     # ... and wrap this one with int_big, not with int
            assert (np.abs(v).max() >= 2.0 ** 31) == (values == "int_big")
        else:
            assert np.abs(v).max() < 2.0 ** 31
