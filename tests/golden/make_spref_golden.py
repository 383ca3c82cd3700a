"""Fixtures of the sparse-indexing tests: tests/golden/spref_<case>.npz, produced by the
REFERENCE's own SpParMat::operator()(ri, ci) (SubsRef_SR, SpParMat.cpp:2026-2247) through
tools/ref_spref_driver.cpp (compile it by the line in its header comment).

    python tests/golden/make_spref_golden.py <path to ref_spref_driver>     (MPIRUN: the launcher, default mpirun)

Each file holds the input matrix (spref_ref.golden_input) as triples in_row, in_col, in_val
with its shape m, n, the index vectors ri, ci (spref_ref.golden_case) and the reference's
result as (column, row)-sorted triples out_row, out_col, out_val.  The reference runs at 1
and at 4 ranks, and the two runs must agree by bits; a case on which the reference aborts or
disagrees with itself at 4 ranks is recorded from the 1-rank run alone and named in `ranks`
(DESIGN.md says which and why).  Every result is also compared with the restatement.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hipmcl_ref as hr  # noqa: E402
import spref_ref as sr  # noqa: E402
from make_mcl_golden import write_mtx  # noqa: E402

RANKS = (1, 4)


def run_reference(driver, mtx, ri, ci, symmetric, ranks, tmp):
    out = os.path.join(tmp, "out")
    for name, v in (("ri.txt", ri), ("ci.txt", ci)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write("%d\n" % len(v) + "\n".join(str(int(x)) for x in v) + "\n")
    cmd = [driver, mtx, os.path.join(tmp, "ri.txt"), os.path.join(tmp, "ci.txt"), "1" if symmetric else "0", out]
    if ranks > 1:
        cmd = [os.environ.get("MPIRUN", "mpirun"), "-n", str(ranks)] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       env=dict(os.environ, OMP_NUM_THREADS="1"), timeout=300)
    if r.returncode != 0:
        return None, r.stdout[-2000:]
    rows = []
    for k in range(ranks):
        p = f"{out}.r{k}"
        if os.path.getsize(p):
            rows.append(np.loadtxt(p, ndmin=2))
        os.remove(p)
    a = np.concatenate(rows) if rows else np.zeros((0, 3))
    o = np.lexsort((a[:, 0], a[:, 1]))
    return (a[o, 0].astype(np.int64), a[o, 1].astype(np.int64), a[o, 2].astype(np.float64)), ""


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


def main():
    driver = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        mtx = os.path.join(tmp, "in.mtx")
        for name in sr.GOLDEN_CASES:
            t, ri, ci = sr.golden_case(name)
            write_mtx(mtx, t)
            want = sr.spref(t, ri, ci)
            want = (want["ir"].astype(np.int64), hr.cols_of(want), want["val"])
            one, log = run_reference(driver, mtx, ri, ci, name == "symperm", 1, tmp)
            assert one is not None, (name, log)
            ran = [1]
            for ranks in RANKS[1:]:
                more, log = run_reference(driver, mtx, ri, ci, name == "symperm", ranks, tmp)
                if more is None:
                    print(name, "the reference failed at", ranks, "ranks:", log[-400:])
                elif not same(one, more):
                    print(name, "the reference at", ranks, "ranks disagrees with its 1-rank run:", len(more[0]), "entries against", len(one[0]))
                else:
                    ran.append(ranks)
            assert same(one, want), (name, "the restatement disagrees with the reference")
            np.savez_compressed(os.path.join(HERE, f"spref_{name}.npz"), m=t["m"], n=t["n"],
                                in_row=t["ir"].astype(np.int64), in_col=hr.cols_of(t), in_val=t["val"],
                                ri=np.asarray(ri, np.int64), ci=np.asarray(ci, np.int64), out_row=one[0], out_col=one[1],
                                out_val=one[2], ranks=np.asarray(ran))
            print(name, "entries", len(one[0]), "ranks agreed", ran)


if __name__ == "__main__":
    main()
