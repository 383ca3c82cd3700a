"""The big-column cut chosen per multiply (csrc/cbg_local.hip, LOW_CUT_FLOPS): the columns of
1025-4096 flops join the big-column path where (a) m <= 2^22 rows and (b) the columns above
4096 flops carry at least half of the multiply's flops; CBG_BIG_FLOPS overrides the rule.
Every product is compared with the CPU oracle entry by entry (integer values: exact in any
order), in both semirings; which side of the rule an input falls on is worked out on the CPU
from the oracle's flops per column before the device is asked."""
import functools

import numpy as np
import pytest

import helpers as H
from helpers import assert_tiles_equal, oracle_local, oracle_symbolic

pytestmark = pytest.mark.gpu

SPAN = 1 << 22  # GRANK_SPAN_LOG: rows a whole-column group's rank slab can span


def _rule(Ah, Bh):
    """the cut the rule takes and the share of the flops in columns above 4096 flops
    (thin and single-entry columns counted as the library's histogram counts them: thin
    ones with the big columns, single-entry ones with neither)"""
    f = np.asarray(oracle_symbolic(Ah, Bh)[0], np.int64)
    nb = np.diff(Bh["cp"])
    share = float(f[(f > 4096) & (nb > 1)].sum()) / float(f.sum())
    moved = int(((f > 1024) & (f <= 4096) & (nb > 1)).sum())
    low = Ah["m"] <= SPAN and 2 * int(f[(f > 4096) & (nb > 1)].sum()) >= int(f.sum()) and moved > 0
    return (1024 if low else 4096), share, f, nb


def _n_big(Ah, f, nb, cut):
    """k_classify's big columns at `cut`: more flops, more than one B entry, not thin"""
    R = (Ah["m"] + H.PANEL - 1) // H.PANEL
    big = (f > cut) & (nb > 1)
    thin = big & (R >= 4) & (f * 4 < nb * R)
    return int((big & ~thin).sum()), int(thin.sum())


@functools.lru_cache(maxsize=None)
def _rmat14():
    A = H.oracle_rmat(14, 16)
    return A, dict(A)


@functools.lru_cache(maxsize=None)
def _hubs_and_mid_columns():
    """400 columns of 1500 flops (15 A columns of 100 rows) and 3 columns of 5200 flops (a
    5000-row hub and two ordinary A columns) over m = 2^19 + 5 rows (3 row panels): the
    columns above 4096 flops carry 2.5 % of the flops"""
    rng = np.random.default_rng(23)
    m, nheavy, nhub = (1 << 19) + 5, 300, 3
    lens = [100] * nheavy + [5000] * nhub
    Ah = H.sparse_cols(rng, m, lens)
    Ah["val"] = rng.integers(1, 5, len(Ah["ir"])).astype(np.float64)
    bcols = [np.sort(rng.choice(nheavy, 15, replace=False)) for _ in range(400)]
    bcols += [np.sort(np.append(rng.choice(nheavy, 2, replace=False), nheavy + h)) for h in range(nhub)]
    bc = np.array([len(c) for c in bcols])
    Bh = dict(m=len(lens), n=len(bcols), cp=np.concatenate([[0], np.cumsum(bc)]).astype(np.int64),
              jc=np.arange(len(bcols), dtype=np.int32), ir=np.concatenate(bcols).astype(np.int32),
              val=rng.integers(1, 3, int(bc.sum())).astype(np.float64))
    return Ah, Bh


@functools.lru_cache(maxsize=None)
def _panels65():
    return H.panel_group_operands((1 << 24) + 77)


@functools.lru_cache(maxsize=None)
def _reference(name, sr):
    Ah, Bh = OPERANDS[name]()
    return oracle_local(Ah, Bh, sr)


OPERANDS = {"rmat14": _rmat14, "hubs_mid": _hubs_and_mid_columns, "panels65": _panels65}


def _run(cbg, name, sr):
    Ah, Bh = OPERANDS[name]()
    A, B = cbg.Tile.from_dict(Ah), cbg.Tile.from_dict(Bh)
    C = cbg.LocalHybridSpGEMM(A, B, sr)
    st, w = cbg.last_stats(), {k: int(v) for k, v in cbg.last_work_stats().items()}
    Ch = C.to_host()
    for t in (A, B, C):
        t.free()
    print(name, sr, st["n_big"], {k: v for k, v in w.items() if v})
    assert_tiles_equal(Ch, _reference(name, sr))
    return st, w


@pytest.fixture
def no_override(monkeypatch):
    monkeypatch.delenv("CBG_BIG_FLOPS", raising=False)
    monkeypatch.delenv("CBG_THIN", raising=False)


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_rule_takes_the_low_cut_on_rmat14(cbg, sr, no_override):
    """(a) and (b) hold: the cut is 1024 and n_big counts the 1025-4096-flop columns"""
    Ah, Bh = _rmat14()
    cut, share, f, nb = _rule(Ah, Bh)
    assert cut == 1024 and share >= 0.5 and Ah["m"] <= SPAN, share
    n4096, n1024 = _n_big(Ah, f, nb, 4096)[0], _n_big(Ah, f, nb, 1024)[0]
    assert n1024 > n4096 > 0
    st, w = _run(cbg, "rmat14", sr)
    assert w["big_cut_flops"] == 1024 and st["n_big"] == n1024, (st, w, n1024)


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_rule_keeps_4096_where_big_columns_are_few(cbg, sr, no_override):
    """(b) fails: columns above 4096 flops carry 2.5 % of the flops"""
    Ah, Bh = _hubs_and_mid_columns()
    cut, share, f, nb = _rule(Ah, Bh)
    assert cut == 4096 and share < 0.05 and Ah["m"] <= SPAN, share
    assert int(((f > 1024) & (f <= 4096)).sum()) == 400
    st, w = _run(cbg, "hubs_mid", sr)
    assert w["big_cut_flops"] == 4096 and st["n_big"] == 3 == _n_big(Ah, f, nb, 4096)[0], (st, w)
    assert w["hash_bin_columns"] >= 400, w  # the 1500-flop columns stayed in the block hash bins


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_rule_keeps_4096_above_the_rank_slab_span(cbg, sr, no_override):
    """(a) fails at m = 2^24 + 77 although the big columns carry over 90 % of the flops:
    n_big as test_panel_groups_65_panels expects it with the thin pass on"""
    Ah, Bh = _panels65()
    cut, share, f, nb = _rule(Ah, Bh)
    assert cut == 4096 and share > 0.9 and Ah["m"] > SPAN, share
    assert int(((f > 1024) & (f <= 4096) & (nb > 1)).sum()) > 0  # there was something to move
    st, w = _run(cbg, "panels65", sr)
    assert w["big_cut_flops"] == 4096 and st["n_big"] == 300 == _n_big(Ah, f, nb, 4096)[0], (st, w)


@pytest.mark.parametrize("sr", ["plus", "minplus"])
@pytest.mark.parametrize("name,forced", [("rmat14", 4096), ("hubs_mid", 1024)])
def test_override_beats_the_rule(cbg, name, forced, sr, monkeypatch):
    """CBG_BIG_FLOPS set explicitly wins in both directions"""
    Ah, Bh = OPERANDS[name]()
    cut, share, f, nb = _rule(Ah, Bh)
    assert cut != forced
    monkeypatch.delenv("CBG_THIN", raising=False)
    monkeypatch.setenv("CBG_BIG_FLOPS", str(forced))
    st, w = _run(cbg, name, sr)
    want = _n_big(Ah, f, nb, forced)
    assert w["big_cut_flops"] == forced and st["n_big"] == want[0] and w["thin_columns"] == want[1], (st, w, want)


# --------------------------------------------------------------------------
# the rule's thin path: columns of 1025-4096 flops that the lower cut makes thin
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _thin_mid_columns():
    """m = 2^22 - 3 (16 row panels): 30 columns of 20000 flops, 40 of 1500 flops over 15 B
    entries (big at the lower cut) and 25 of 1200 flops over 600 B entries on two-row A
    columns (flops x 4 < entries x 16: thin at the lower cut, block hash columns at 4096)"""
    rng = np.random.default_rng(31)
    m, nheavy, nlight = (1 << 22) - 3, 500, 2000
    Ah = H.sparse_cols(rng, m, [100] * nheavy + [2] * nlight)
    Ah["val"] = rng.integers(1, 5, len(Ah["ir"])).astype(np.float64)
    bcols = [np.sort(rng.choice(nheavy, 200, replace=False)) for _ in range(30)]
    bcols += [np.sort(rng.choice(nheavy, 15, replace=False)) for _ in range(40)]
    bcols += [np.sort(nheavy + rng.choice(nlight, 600, replace=False)) for _ in range(25)]
    bcols = [bcols[i] for i in rng.permutation(len(bcols))]
    return Ah, _b_of(bcols, nheavy + nlight, rng)


def _b_of(bcols, k, rng):
    bc = np.array([len(c) for c in bcols])
    return dict(m=k, n=len(bcols), cp=np.concatenate([[0], np.cumsum(bc)]).astype(np.int64),
                jc=np.arange(len(bcols), dtype=np.int32), ir=np.concatenate(bcols).astype(np.int32),
                val=rng.integers(1, 3, int(bc.sum())).astype(np.float64))


OPERANDS["thin_mid"] = _thin_mid_columns


@pytest.mark.parametrize("sr", ["plus", "minplus"])
def test_rule_moves_thin_columns_to_the_thin_pass(cbg, sr, no_override):
    Ah, Bh = _thin_mid_columns()
    cut, share, f, nb = _rule(Ah, Bh)
    assert cut == 1024 and share >= 0.5, share
    assert _n_big(Ah, f, nb, 4096) == (30, 0) and _n_big(Ah, f, nb, 1024) == (70, 25)
    st, w = _run(cbg, "thin_mid", sr)
    assert w["big_cut_flops"] == 1024 and st["n_big"] == 70 and w["thin_columns"] == 25, (st, w)
