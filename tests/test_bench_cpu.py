"""bench.py host logic without a GPU: the N>1 transport rule and the per-rank roofline
(Weak 6: an N>1 line must neither report the fastest rank's bandwidth nor
fall back to the TCP host transport silently)."""
import importlib.util
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_rccl_failure_exits_nonzero_without_opt_in():
    b = load_bench()
    with pytest.raises(SystemExit) as e:
        b.host_transport_fallback(3, RuntimeError("ncclCommInitRank failed"), env={})
    assert e.value.code not in (0, None)  # a message: exit status 1
    assert "CBG_ALLOW_HOST_TRANSPORT" in str(e.value.code)
    # opted in: no exit, the caller continues on the host transport
    b.host_transport_fallback(3, RuntimeError("x"), env={"CBG_ALLOW_HOST_TRANSPORT": "1"})


def test_rccl_failure_exit_status_of_a_process():
    """the same rule seen from outside: the interpreter exits with status 1"""
    code = ("import importlib.util,sys;s=importlib.util.spec_from_file_location('b',%r);"
            "m=importlib.util.module_from_spec(s);s.loader.exec_module(m);"
            "m.host_transport_fallback(0, RuntimeError('no RCCL'))") % os.path.join(REPO, "bench.py")
    env = {k: v for k, v in os.environ.items() if k != "CBG_ALLOW_HOST_TRANSPORT"}
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "not falling back" in r.stderr


def test_roofline_over_ranks_uses_the_slowest_rank():
    b = load_bench()
    # rank 1 is slow: the job's per-GPU rate is all bytes over rank 1's time / N
    r = b.roofline_over_ranks([100e9, 100e9], [50.0, 100.0], 2, 8000.0)
    assert r["slowest_rank"] == 1
    assert r["achieved"] == pytest.approx(200e9 / 0.1 / 2 / 1e9)  # 1000 GB/s per GPU
    assert r["frac"] == pytest.approx(1000.0 / 8000.0)
    assert r["slowest_rank_achieved"] == pytest.approx(100e9 / 0.1 / 1e9)
    # never the fastest rank's rate (2000 GB/s here)
    assert r["achieved"] < 100e9 / 0.05 / 1e9
    # one rank: the plain rate
    one = b.roofline_over_ranks([1.22e12], [430.0], 1, 8000.0)
    assert one["achieved"] == pytest.approx(1.22e12 / 0.43 / 1e9)


def test_default_grids_and_flags():
    b = load_bench()
    assert b.GRIDS[1] == (1, 1) and b.GRIDS[2][0] * b.GRIDS[2][1] == 2 and b.GRIDS[8][0] * b.GRIDS[8][1] == 8
    src = open(os.path.join(REPO, "bench.py")).read()
    assert "--no-f64-leg" in src and "frac_f64_values" in src


def test_plain_run_flags():
    """a plain run times the headline only: what takes runs of its own sits behind --full"""
    b = load_bench()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
        a = b.parse()
        assert not a.full and a.dump_outputs is None and a.steps == 3
        sys.argv = ["bench.py", "--full", "--dump-outputs", "d", "--no-f64-leg"]
        a = b.parse()
        assert a.full and a.dump_outputs == "d" and not a.f64_leg
        sys.argv = ["bench.py", "--steps", "0"]
        with pytest.raises(SystemExit):
            b.parse()
    finally:
        sys.argv = argv


class _HostTiles:
    """stands in for the binding: cbg_tile_download copies from host arrays"""

    def __init__(self, cbg):
        self.CTile = cbg.CTile

    def lib(self):
        return self

    def _check(self, rc):
        assert rc == 0

    def cbg_tile_download(self, d, h):
        import ctypes
        d, h = d._obj, h._obj
        assert d.on_device and 0 <= d.nzc <= d.n
        ctypes.memmove(h.cp, d.cp, 8 * (d.nzc + 1))
        if d.nzc:
            ctypes.memmove(h.jc, d.jc, 4 * d.nzc)
        if d.nnz:
            ctypes.memmove(h.ir, d.ir, 4 * d.nnz)
            ctypes.memmove(h.val, d.val, 8 * d.nnz)
        return 0


def test_output_sample_is_independent_of_the_phase_cuts(cbg, tmp_path):
    """--dump-outputs: the sample of C is the same whether C arrives as one tile or as
    column phases cut anywhere (a cut inside a sampled run included), holds C's own
    entries, and keeps at most BLOCK_CAP entries of a run"""
    import numpy as np
    b = load_bench()
    rng = np.random.default_rng(7)
    m, n = 1000, 4099
    counts = rng.integers(0, 40, n) * (rng.random(n) < 0.7)  # ~30 % empty columns
    counts[n // 2:] //= 8  # light columns: their runs stay under the cap
    cols = {j: np.sort(rng.choice(m, int(k), replace=False)).astype(np.int32) for j, k in enumerate(counts) if k}
    vals = {j: rng.random(len(r)) for j, r in cols.items()}

    class Tile:  # a DCSC tile of columns [c0, c1), arrays kept alive on the object
        def __init__(self, c0, c1):
            js = [j for j in range(c0, c1) if j in cols]
            self.jc = np.array([j - c0 for j in js] or [0], np.int32)
            self.cp = np.concatenate([[0], np.cumsum([len(cols[j]) for j in js])]).astype(np.int64)
            self.ir = np.concatenate([cols[j] for j in js] or [np.zeros(1, np.int32)])
            self.val = np.concatenate([vals[j] for j in js] or [np.zeros(1)])
            self.c = cbg.CTile(m, c1 - c0, int(self.cp[-1]), len(js), self.cp.ctypes.data, self.jc.ctypes.data,
                               self.ir.ctypes.data, self.val.ctypes.data, 1, 0)

    class Sample(b.OutputSample):
        BLOCKS, BLOCK_COLS, BLOCK_CAP = 8, 16, 200

    fake = _HostTiles(cbg)
    nz = sorted(cols)
    starts = Sample(len(nz)).starts
    assert starts[-1] + Sample.BLOCK_COLS <= len(nz)
    out = {}
    for name, cuts in (("one", [0, n]), ("three", [0, nz[starts[0] + 3] + 1, 2500, n]), ("empty", [0, 1, 2, 3000, n])):
        s = Sample(len(nz))
        for c0, c1 in zip(cuts[:-1], cuts[1:]):
            s.take(fake, 100, 2000 + c0, Tile(c0, c1))
        assert s.seen == len(nz)
        s.save(str(tmp_path / name), "", [1.0, 2.0, 3.0])
        out[name] = {f[:-4]: np.load(str(tmp_path / name / f)) for f in sorted(os.listdir(str(tmp_path / name)))}
    # the same sample from the matrix itself
    want = {"sample_cols": [], "sample_col_nnz": [], "sample_ptr": [0], "sample_rows": [], "sample_vals": []}
    capped = 0
    for st in starts:
        room = Sample.BLOCK_CAP
        for j in nz[st:st + Sample.BLOCK_COLS]:
            k = min(len(cols[j]), room)
            room -= k
            want["sample_cols"].append(2000 + j)
            want["sample_col_nnz"].append(len(cols[j]))
            want["sample_ptr"].append(want["sample_ptr"][-1] + k)
            want["sample_rows"] += list(cols[j][:k] + 100)
            want["sample_vals"] += list(vals[j][:k])
        capped += room == 0
    assert 0 < capped < Sample.BLOCKS  # runs cut by the cap and whole runs
    want["totals"] = [1.0, 2.0, 3.0]
    for name, got in out.items():
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k].dtype == np.float64 and np.array_equal(got[k], np.array(v, np.float64)), (name, k)


def test_newest_profile_lookup(tmp_path):
    """the CPU-baseline and traffic records come from the highest round present
    (a hard-coded round list skipped r04)"""
    import json
    b = load_bench()
    for rnd, v in (("r02", 65.6e6), ("r04", 68.9e6), ("r10", 70.0e6), ("r03", 1.0)):
        (tmp_path / ("%s_cpu_reference_s22.json" % rnd)).write_text(json.dumps({"value": v}))
    (tmp_path / "r11_cpu_reference_s22.json").write_text("not json")
    d, path = b.newest_profile("cpu_reference_s22.json", lambda d: "value" in d, root=str(tmp_path))
    assert d["value"] == 70.0e6 and path.endswith("r10_cpu_reference_s22.json")
    # a predicate skips records of other configurations
    d, _ = b.newest_profile("cpu_reference_s22.json", lambda d: d["value"] < 69e6, root=str(tmp_path))
    assert d["value"] == 68.9e6
    # the committed records: the newest round's s22 reference run
    s22 = b.cpu_baseline_s22()
    rounds = sorted(int(n[1:3]) for n in os.listdir(os.path.join(REPO, "profiles"))
                    if n.endswith("_cpu_reference_s22.json"))
    assert s22["source"] == "profiles/r%02d_cpu_reference_s22.json" % rounds[-1]
