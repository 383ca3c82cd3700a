"""Fixtures of the HipMCL tests: tests/golden/hipmcl_<case>.npz, produced by the
REFERENCE's own Applications/MCL.cpp through tools/ref_hipmcl_driver.cpp (compile it
by the line in its header comment).

    python tests/golden/make_hipmcl_golden.py <path to ref_hipmcl_driver>     (MPIRUN: the launcher, default mpirun)

Each file holds one input matrix of tests/hipmcl_ref.CASES and, for every parameter
set k of hipmcl_ref.PARAM_SETS, the reference's results as sorted (col, row, value)
triples: adjust<k> (AdjustLoops), stoch<k> (MakeColStochastic of that), inflate<k>
(Inflate(power) of that), chaos<k> (Chaos of the stochastic matrix); and the labels
of Interpret(input) and of HipMCL(input) (canonically renumbered: the reference's
numbering follows LACC's internals), HipMCL's iteration count and the 3-digit chaos
values of its printed lines.  The reference runs at 1 and at 4 ranks; the two runs
must agree on every dump, on the labels and on the iteration count.

Asserted here through the restatement: selection and recovery both fire in some
iteration (where S > 0), and the partition and iteration count survive a relative
1e-12 perturbation of every input weight (the device multiply accumulates in another
order than any host code, so the cases must not sit on a knife edge).
"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hipmcl_ref as hr  # noqa: E402
from make_mcl_golden import write_mtx  # noqa: E402

# Rank counts the reference runs at: every case at 1 and 4, and the runs must agree.  They do
# only while no squared operand has a column longer than hipmcl_ref.REF_SCAN_LIMIT entries
# (see there: the reference's unsorted hash kernels against Dcsc::FillColInds' scanning
# path); main() asserts that limit for every case through the restatement.
RANKS = (1, 4)

ITER = re.compile(r"Iteration#\s+(\d+)\s*:\s+chaos:\s*(\S+)")


def _triples(prefix, what, ranks):
    rows = []
    for r in range(ranks):
        p = f"{prefix}.{what}.r{r}"
        if os.path.getsize(p):
            rows.append(np.loadtxt(p, ndmin=2))
        os.remove(p)
    a = np.concatenate(rows) if rows else np.zeros((0, 3))
    o = np.lexsort((a[:, 0], a[:, 1]))
    return a[o, 1].astype(np.int32), a[o, 0].astype(np.int32), a[o, 2].astype(np.float64)


def _labels(prefix, what, ranks, n):
    lab = np.full(n, -1, np.int64)
    for r in range(ranks):
        p = f"{prefix}.{what}.r{r}"
        if os.path.getsize(p):
            a = np.loadtxt(p, ndmin=2).astype(np.int64)
            lab[a[:, 0]] = a[:, 1]
        os.remove(p)
    assert lab.min() >= 0
    return hr.canonical(lab)


def run_reference(driver, mtx, ps, ranks, tmp, n):
    infl, h, S, R, q = ps
    out = os.path.join(tmp, "out")
    cmd = [driver, mtx, repr(float(infl)), repr(float(h)), str(S), str(R), repr(float(q)), out]
    if ranks > 1:
        cmd = [os.environ.get("MPIRUN", "mpirun"), "-n", str(ranks)] + cmd
    r = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, OMP_NUM_THREADS="1"))  # SpParHelper::Print writes to stderr
    res = {w: _triples(out, w, ranks) for w in ("adjust", "stoch", "inflate")}
    res["interpret"] = _labels(out, "interpret", ranks, n)
    res["hipmcl"] = _labels(out, "hipmcl", ranks, n)
    res["chaos"] = float(open(out + ".scalars").read().split()[1])
    its = ITER.findall(r.stdout)
    assert its and [int(i) for i, _ in its] == list(range(1, len(its) + 1)), r.stdout[-2000:]
    res["iterations"] = len(its)
    res["printed"] = np.array([float(c) for _, c in its])
    return res


def main():
    driver = os.path.abspath(sys.argv[1])
    for name, make in hr.CASES.items():
        t = make()
        save = dict(m=t["m"], n=t["n"], cp=t["cp"], jc=t["jc"], ir=t["ir"], val=t["val"],
                    params=np.asarray(hr.PARAM_SETS, np.float64), ranks=np.asarray(RANKS))
        rng = np.random.default_rng(0)
        with tempfile.TemporaryDirectory() as tmp:
            mtx = os.path.join(tmp, "in.mtx")
            write_mtx(mtx, t)
            for k, ps in enumerate(hr.PARAM_SETS):
                took = {}
                lab, it, ch, _ = hr.hipmcl(t, *ps, took=took)
                if ps[2] > 0:
                    assert took["selection"] and (took["recovery"] or took["recovery_after_selection"]), (name, ps)
                assert took["longest_column"] <= hr.REF_SCAN_LIMIT, (name, ps, took["longest_column"])
                p = dict(t, val=t["val"] * (1.0 + 1e-12 * rng.uniform(-1, 1, len(t["val"]))))
                lab2, it2, _, _ = hr.hipmcl(p, *ps)
                assert it2 == it and np.array_equal(lab, lab2), (name, ps, "not robust: pick another seed")
                one = run_reference(driver, mtx, ps, 1, tmp, t["n"])
                for ranks in RANKS[1:]:
                    more = run_reference(driver, mtx, ps, ranks, tmp, t["n"])
                    for w in ("adjust", "stoch", "inflate"):
                        for a, b in zip(one[w][:2], more[w][:2]):
                            assert np.array_equal(a, b), (name, ps, w)
                        assert np.allclose(one[w][2], more[w][2], rtol=1e-14, atol=0), (name, ps, w)
                    assert np.array_equal(one["hipmcl"], more["hipmcl"]), (name, ps, ranks)
                    assert one["iterations"] == more["iterations"], (name, ps, ranks)
                    assert np.array_equal(one["interpret"], more["interpret"])
                for w in ("adjust", "stoch", "inflate"):
                    save[f"{w}{k}_col"], save[f"{w}{k}_row"], save[f"{w}{k}_val"] = one[w]
                save[f"chaos{k}"] = one["chaos"]
                save[f"labels{k}"] = one["hipmcl"]
                save[f"iterations{k}"] = one["iterations"]
                save[f"printed{k}"] = one["printed"]
                save["interpret"] = one["interpret"]
                print(name, ps, "iterations", one["iterations"], "clusters", int(one["hipmcl"].max()) + 1,
                      "restatement", it, int(lab.max()) + 1)
        np.savez_compressed(os.path.join(HERE, f"hipmcl_{name}.npz"), **save)


if __name__ == "__main__":
    main()
