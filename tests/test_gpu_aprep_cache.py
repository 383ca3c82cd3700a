"""The A-side preparation one phased multiply keeps for all its pieces (csrc/cbg_local.hip
APrep: A's column map, the R x (n+1) panel map, A's values as f32 / (row, f32) / (row, f64)
records, the f32-exact and integral verdicts and max |a|), across pieces that are NOT alike.

Every other phased test multiplies R-MAT by R-MAT: all pieces take the route the first one
took.  Here B is a sequence of unlike blocks (helpers.APREP_SEQUENCES; tests/
test_aprep_cases_cpu.py shows without a device that each block is its kind), one block per
phase of MemEfficientSpGEMM on a 1x1 grid, and A (m = 2^20 + 77: 5 row panels) takes four
value sets.  The on_phase callback downloads each piece and reads last_work_stats(): the
differences of those running sums are the piece's own counters, so every piece is pinned
twice -- its bits against oracle_local of the host slice, and the route it took
(amap_reused, pmap_reused / pmap_built / pmap_entries, avals_reused, rvd_built / rvd_used,
int_accumulate, big_cut_flops) against what the pieces before it left behind.

An `empty` piece stores no column: the multiply returns before it looks at the cache, and
all its counters are 0 (amap_reused included).

The sample symbolic of the memory plan (PHASES_AUTO: the sym_only multiply that fills the
maps but not the verdicts) needs 12 x flops above the C budget.  perProcessMemory counts whole
GB, so with the default share of it (CBG_PHASE_MEM_FRAC = 0.6) the smallest budget is 5.9e8
bytes, far above the 3.8e7 of sequence (a); test_sample_symbolic_first therefore sets the
share (read once per process: a fresh process) so that the budget asks for one phase per block."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from helpers import assert_tiles_bits_equal

pytestmark = pytest.mark.gpu

ROUTES = ("amap_reused", "pmap_reused", "pmap_built", "pmap_entries", "avals_reused", "rvd_built", "rvd_used")
# kind -> (has big columns, their B entries x entries factor < A's stored columns,
#          their flops >= flops factor x nnz(A)); tests/test_aprep_cases_cpu.py test_block_is_its_kind
KIND = dict(small=(False, None, None), empty=None, lean=(True, True, False), thin=(True, True, False),
            rich=(True, False, True), B_half=(True, False, True), B_zero=(True, False, True),
            B_heavy=(True, False, True))
CASES = [(s, v, sr) for s in sorted(H.APREP_SEQUENCES) for v, srs in H.APREP_A_VALUES.items() for sr in srs]
_RUNS = {}   # (seq, values, sr) -> the streamed PANEL pieces [(phase, offset, host tile, counters)]


def _grid(cbg):
    class Self:
        def bcast(self, comm, arr, root):
            pass

        def allgather(self, comm, data):
            return data

    return cbg.CommGrid(0, 1, transport="host", host_comm=Self())


def _mat(cbg, grid, d):
    return cbg.SpParMat(cbg.Tile.from_dict(d), grid, d["m"], d["n"])


def _phased(cbg, A, B, P, sr, **kw):
    """MemEfficientSpGEMM streamed: [(phase, offset, host tile, this piece's counters)]"""
    out, prev = [], {}

    def on_phase(ph, off, t):
        w = {k: int(v) for k, v in cbg.last_work_stats().items()}
        d = {k: v - prev.get(k, 0) for k, v in w.items()}
        d["big_cut_flops"] = w["big_cut_flops"]      # (a threshold, not a sum: the last multiply's)
        prev.clear()
        prev.update(w)
        out.append((ph, off, t.to_host(), d))

    cbg.MemEfficientSpGEMM(A, B, P, sr, on_phase=on_phase, **kw)
    return out


def _stream(cbg, seq, values, sr):
    key = (seq, values, sr)
    if key not in _RUNS:
        grid = _grid(cbg)
        Bh, kinds = H.aprep_B(seq)
        A, B = _mat(cbg, grid, H.aprep_A(values)), _mat(cbg, grid, Bh)
        try:
            _RUNS[key] = _phased(cbg, A, B, len(kinds), sr)
        finally:
            A.tile.free()
            B.tile.free()
            grid.destroy()
    return _RUNS[key]


def expected_routes(kinds, f64, primed=False):
    """the route of each piece from the pieces before it, with the kinds' properties from
    KIND; primed: the plan's sample symbolic ran first and left both maps (no verdicts)"""
    amap = pmap = primed
    verdict = rvd = False
    out = []
    for kind in kinds:
        e = dict.fromkeys(ROUTES, 0)
        out.append(e)
        if KIND[kind] is None:      # no stored column: no multiply
            continue
        has_big, few_entries, pays_rvd = KIND[kind]
        e["amap_reused"], amap = int(amap), True
        if not has_big:
            continue
        if pmap:
            e["pmap_reused"] = 1
        elif few_entries:
            e["pmap_entries"] = 1   # private: not kept
        else:
            e["pmap_built"], pmap = 1, True
        e["avals_reused"], verdict = int(verdict), True
        if f64 and (rvd or pays_rvd):
            e["rvd_used"], e["rvd_built"], rvd = 1, int(not rvd), True
    return out


def expected_int_accumulate(seq, values, sr):
    """exact int32 accumulation per piece, from the documented rule (include/cbg.h): A's and
    B's values nonzero integers of magnitude <= 2^24, and max|a| x (B's largest column sum
    of |b|) < 2^31 (plus-times) or max|a| + max|b| < 2^30 (min-plus); only slabs accumulate"""
    Bh, kinds = H.aprep_B(seq)
    A = H.aprep_A(values)
    amax = float(np.abs(A["val"]).max())
    out = []
    for kind, Bp in zip(kinds, H.aprep_pieces(Bh, len(kinds))):
        fa = H.aprep_piece_facts(A, Bp)
        ok = values.startswith("int") and fa["nbig"] > 0 and fa["b_integral"]
        bound = amax * fa["b_colsum"] < 2.0 ** 31 if sr == "plus" else amax + fa["b_max"] < 2.0 ** 30
        out.append(int(ok and bound))
    return out


def test_aprep_bounds_are_the_tested_ones(cbg):
    """the thresholds the operands were built against (helpers, used without a device by
    tests/test_aprep_cases_cpu.py) are the library's"""
    assert cbg.local_aprep_bounds() == [H.APREP_ENTRIES, H.APREP_RVD_FLOPS]


@pytest.mark.parametrize("seq,values,sr", CASES)
def test_unlike_pieces_routes_and_bits(cbg, seq, values, sr):
    kinds = H.APREP_SEQUENCES[seq]
    got = _stream(cbg, seq, values, sr)
    refs = H.aprep_refs(seq, values, sr)
    assert [(ph, off) for ph, off, _, _ in got] == [(p, p * H.APREP_W) for p in range(len(kinds))]
    Bh = H.aprep_B(seq)[0]
    facts = [H.aprep_piece_facts(H.aprep_A(values), Bp) for Bp in H.aprep_pieces(Bh, len(kinds))]
    want = expected_routes(kinds, values == "f64")
    iacc = expected_int_accumulate(seq, values, sr)
    for p, kind in enumerate(kinds):
        C, w = got[p][2], got[p][3]
        print(seq, values, sr, p, kind, {k: v for k, v in w.items() if v})
        assert_tiles_bits_equal(C, refs[p])
        assert {k: w[k] for k in ROUTES} == want[p], (p, kind)
        assert w["int_accumulate"] == iacc[p], (p, kind, w)
        assert w["big_cut_flops"] == facts[p]["cut"], (p, kind, w)
        assert (w["thin_columns"] > 0) == (kind == "thin"), (p, kind, w)
    # the rich pieces ran panel groups, hash slabs and bitmap slabs
    for p, kind in enumerate(kinds):
        if kind in H.APREP_RICH_LIKE:
            w = got[p][3]
            assert w["sym_group_units"] > 0 and w["sym_panel_units"] > 0, (p, w)
            assert sum(v for k, v in w.items() if k.startswith("hash_T")) > 0, (p, w)
            assert sum(v for k, v in w.items() if k.startswith("bitmap_")) > 0, (p, w)


def test_sequence_a_routes_as_stated(cbg):
    """sequence (a) = small, lean, rich, lean, empty, rich, thin with the f64 values, spelled
    out: the lean piece before any rich one maps only its entries and packs nothing, the
    first rich one builds the panel map and packs the (row, f64) records, every later piece
    with big columns reuses both -- the lean one too, however small"""
    assert H.APREP_SEQUENCES["a"] == ["small", "lean", "rich", "lean", "empty", "rich", "thin"]
    w = [x[3] for x in _stream(cbg, "a", "f64", "plus")]
    col = lambda k: [x[k] for x in w]   # noqa: E731
    assert col("amap_reused") == [0, 1, 1, 1, 0, 1, 1]
    assert col("pmap_entries") == [0, 1, 0, 0, 0, 0, 0]
    assert col("pmap_built") == [0, 0, 1, 0, 0, 0, 0]
    assert col("pmap_reused") == [0, 0, 0, 1, 0, 1, 1]
    assert col("avals_reused") == [0, 0, 1, 1, 0, 1, 1]
    assert col("rvd_built") == [0, 0, 1, 0, 0, 0, 0]
    assert col("rvd_used") == [0, 0, 1, 1, 0, 1, 1]
    for values in ("int", "int_big", "f32"):
        w = [x[3] for x in _stream(cbg, "a", values, "plus")]
        assert [x["rvd_built"] + x["rvd_used"] for x in w] == [0] * 7, values


@pytest.mark.parametrize("values,want", [("int", [0, 0, 0, 1, 0, 1, 1, 1]), ("int_big", [0, 0, 0, 1, 0, 1, 0, 1]),
                                         ("f32", [0] * 8), ("f64", [0] * 8)])
def test_sequence_c_int_accumulate_as_stated(cbg, values, want):
    """sequence (c) = small, small, B_half, rich, B_zero, rich, B_heavy, rich, plus-times: int32
    accumulation is on for rich, off for B_half and B_zero, and for B_heavy on with `int`
    (4 x 2^20 < 2^31) and off with `int_big` (2^24 x 2^20), then on again"""
    assert H.APREP_SEQUENCES["c"] == ["small", "small", "B_half", "rich", "B_zero", "rich", "B_heavy", "rich"]
    got = _stream(cbg, "c", values, "plus")
    assert [x[3]["int_accumulate"] for x in got] == want
    for (_, _, C, _), ref in zip(got, H.aprep_refs("c", values, "plus")):
        assert_tiles_bits_equal(C, ref)


@pytest.mark.parametrize("values", ["int", "f64"])
def test_oom_halves_share_the_scope(cbg, values):
    """sequence (a) with pieces whose C does not fit (CBG_FAULT_C_BYTES, read per call): the
    rich pieces are computed as column halves inside the same scope; the pieces at their
    offsets are the oracle's C"""
    kinds = H.APREP_SEQUENCES["a"]
    refs = H.aprep_refs("a", values, "plus")
    grid = _grid(cbg)
    A, B = _mat(cbg, grid, H.aprep_A(values)), _mat(cbg, grid, H.aprep_B("a")[0])
    os.environ["CBG_FAULT_C_BYTES"] = str(12 * max(len(r["ir"]) for r in refs) // 3)
    try:
        got = _phased(cbg, A, B, len(kinds), "plus")
    finally:
        del os.environ["CBG_FAULT_C_BYTES"]
        plan = cbg.phase_plan()
        A.tile.free()
        B.tile.free()
        grid.destroy()
    assert plan["oom_splits"] >= 1 and len(got) > len(kinds), plan
    got.sort(key=lambda x: x[1])
    offs = [x[1] for x in got]
    assert offs == [0] + list(np.cumsum([x[2]["n"] for x in got])[:-1])
    assert [x[0] for x in got] == [off // H.APREP_W for off in offs]      # each half under its phase's index
    assert_tiles_bits_equal(H.concat_cols_host([x[2] for x in got]), H.concat_cols_host(refs))


def test_scope_ends_with_the_call(cbg):
    """nothing of one call's A survives into the next: after a call with the `int` values that
    A is freed and the `f64` one uploaded (the pool usually hands out the same blocks), and
    the second call starts from nothing; a plain LocalHybridSpGEMM afterwards, outside any
    scope, reuses nothing either"""
    kinds = H.APREP_SEQUENCES["a"]
    Bh = H.aprep_B("a")[0]
    grid = _grid(cbg)
    B = _mat(cbg, grid, Bh)
    A = _mat(cbg, grid, H.aprep_A("int"))
    first = _phased(cbg, A, B, len(kinds), "plus")
    A.tile.free()
    A = _mat(cbg, grid, H.aprep_A("f64"))
    second = _phased(cbg, A, B, len(kinds), "plus")
    for got, values in ((first, "int"), (second, "f64")):
        for (_, _, C, _), ref in zip(got, H.aprep_refs("a", values, "plus")):
            assert_tiles_bits_equal(C, ref)
        assert [{k: x[3][k] for k in ROUTES} for x in got] == expected_routes(kinds, values == "f64"), values
    w = [x[3] for x in second]
    big1 = next(p for p, k in enumerate(kinds) if KIND[k] and KIND[k][0])
    assert w[0]["amap_reused"] == 0 and w[big1]["avals_reused"] == 0 and w[big1]["pmap_reused"] == 0
    # outside any scope: a lean piece maps its entries, a rich one builds the map and packs, nothing is reused
    pieces = H.aprep_pieces(Bh, len(kinds))
    for p in (kinds.index("lean"), kinds.index("rich"), kinds.index("lean")):
        Bp = cbg.Tile.from_dict(pieces[p])
        C = cbg.LocalHybridSpGEMM(A.tile, Bp)
        w1 = {k: int(v) for k, v in cbg.last_work_stats().items()}
        assert_tiles_bits_equal(C.to_host(), H.aprep_refs("a", "f64", "plus")[p])
        rich = kinds[p] == "rich"
        assert {k: w1[k] for k in ROUTES} == dict(amap_reused=0, pmap_reused=0, avals_reused=0, pmap_built=int(rich),
                                                  pmap_entries=int(not rich), rvd_built=int(rich),
                                                  rvd_used=int(rich)), (p, w1)
        C.free()
        Bp.free()
    A.tile.free()
    B.tile.free()
    grid.destroy()


@pytest.mark.parametrize("values", ["int", "f64"])
def test_staged_and_concatenated_controls(cbg, values):
    """sequence (a) through EXEC_STAGED (no cache: its stages multiply different A slices)
    and through the concatenating form gives the bits of the streamed PANEL pieces"""
    kinds = H.APREP_SEQUENCES["a"]
    P = len(kinds)
    panel = [x[2] for x in _stream(cbg, "a", values, "plus")]
    grid = _grid(cbg)
    A, B = _mat(cbg, grid, H.aprep_A(values)), _mat(cbg, grid, H.aprep_B("a")[0])
    try:
        staged = _phased(cbg, A, B, P, "plus", exec_mode=cbg.EXEC_STAGED)
        assert [x[1] for x in staged] == [p * H.APREP_W for p in range(P)]
        for (_, _, C, w), want in zip(staged, panel):
            assert_tiles_bits_equal(C, want)
            assert w["amap_reused"] == w["pmap_reused"] == w["avals_reused"] == 0, w
        whole = H.concat_cols_host(panel)
        for mode in (cbg.EXEC_PANEL, cbg.EXEC_STAGED):
            C = cbg.MemEfficientSpGEMM(A, B, P, "plus", exec_mode=mode)
            assert_tiles_bits_equal(C.tile.to_host(), whole)
            C.tile.free()
    finally:
        A.tile.free()
        B.tile.free()
        grid.destroy()


_SAMPLE_CODE = r"""
import json
import sys
from conftest import load_cbg
import helpers as H
import test_gpu_aprep_cache as T
cbg = load_cbg()
values = sys.argv[1]
grid = T._grid(cbg)
A, B = T._mat(cbg, grid, H.aprep_A(values)), T._mat(cbg, grid, H.aprep_B("a")[0])
got = T._phased(cbg, A, B, cbg.PHASES_AUTO, "plus", perProcessMemory=1)
plan = cbg.phase_plan()
refs = H.aprep_refs("a", values, "plus")
assert len(got) == len(refs), (len(got), plan)
for (ph, off, C, w), ref in zip(got, refs):
    H.assert_tiles_bits_equal(C, ref)
print(json.dumps(dict(plan=plan, pieces=[(ph, off, w) for ph, off, C, w in got])))
"""


@pytest.mark.parametrize("values", ["int", "f64"])
def test_sample_symbolic_first(cbg, values):
    """sequence (a) under the memory plan: the sample (B's columns whose id is a multiple of
    256: column 0 of every block, four of them big) runs the symbolic alone first, inside the
    call's scope.  It leaves A's column map and the full panel map -- so the first piece
    reuses the column map, and the lean piece, the first with big columns, reuses the panel
    map instead of mapping its entries -- but no verdict: that piece checks A's values itself.
    The pieces match the oracle by bits (in the child process)."""
    kinds = H.APREP_SEQUENCES["a"]
    P = len(kinds)
    Ah, Bh = H.aprep_A(values), H.aprep_B("a")[0]
    f, z = H.oracle_symbolic(Ah, Bh)
    keep = Bh["jc"] % 256 == 0
    ratio = min(1.0, 1.1 * float(z[keep].sum()) / float(f[keep].sum()))     # plan_phases' estimate
    tbytes = lambda t: 8 * (len(t["jc"]) + 1) + 4 * len(t["jc"]) + 12 * len(t["ir"])   # noqa: E731
    budget = 12.0 * ratio * float(f.sum()) / (P - 0.5)      # ceil(need / budget) = P
    frac = budget / (1e9 - tbytes(Ah) - tbytes(Bh))
    assert 0 < frac < 1 and 12.0 * float(f.sum()) > budget
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", "import sys\nsys.path.insert(0, %r)\n" % tests + _SAMPLE_CODE, values],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, CBG_PHASE_MEM_FRAC=repr(frac)))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().splitlines()[-1])
    plan = res["plan"]
    assert plan["automatic"] and plan["phases"] == P and plan["flops"] == int(f.sum()), plan
    # (12 x flops exceeds the budget, so the sample was taken; these operands hardly compress, and the
    # estimate may equal the flops: that it ran shows in the first piece's reused column map below)
    assert plan["nnz_est"] == int(ratio * plan["flops"]) and 12.0 * plan["flops"] > plan["c_budget_bytes"], plan
    assert [(ph, off) for ph, off, _ in res["pieces"]] == [(p, p * H.APREP_W) for p in range(P)]
    w = [x[2] for x in res["pieces"]]
    assert [{k: x[k] for k in ROUTES} for x in w] == expected_routes(kinds, values == "f64", primed=True)
    big1 = kinds.index("lean")
    assert w[0]["amap_reused"] == 1 and w[big1]["avals_reused"] == 0 and w[big1]["pmap_reused"] == 1
    assert w[big1]["pmap_entries"] == 0 and [x["pmap_built"] for x in w] == [0] * P
