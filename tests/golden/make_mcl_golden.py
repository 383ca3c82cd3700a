"""Fixtures of the pruning tests: tests/golden/mcl_<case>.npz, produced by the
REFERENCE's own MCLPruneRecoverySelect through tools/ref_mcl_driver.cpp (compile it
by the line in its header comment).

    python tests/golden/make_mcl_golden.py <path to ref_mcl_driver> [ranks ...]     (MPIRUN: the launcher, default mpirun)

Each file holds one input matrix (about 64 x 48, values multiples of 2^-10, every
branch of the algorithm taken by some column under some parameter set: asserted
here) and, for every parameter set of tests/mcl_ref.PARAM_SETS, the reference's
output as sorted (col, row, value) triples.  Runs at 1 rank, and at the other
rank counts given (square grids); their outputs must be identical to the 1-rank one.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mcl_ref  # noqa: E402

CASES = {"a": 11, "b": 23}  # name -> seed of mcl_ref.small_case


def write_mtx(path, t):
    cnt = np.diff(t["cp"])
    col = np.repeat(t["jc"].astype(np.int64), cnt)
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{t['m']} {t['n']} {len(col)}\n")
        for r, c, v in zip(t["ir"], col, t["val"]):
            f.write(f"{int(r) + 1} {int(c) + 1} {float(v)!r}\n")


def run_reference(driver, mtx, params, ranks, tmp):
    h, S, R, q = params
    out = os.path.join(tmp, "out.txt")
    cmd = [driver, mtx, repr(float(h)), str(S), str(R), repr(float(q)), out]
    if ranks > 1:
        cmd = [os.environ.get("MPIRUN", "mpirun"), "-n", str(ranks)] + cmd
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    rows = []
    for r in range(ranks):
        p = f"{out}.r{r}"
        if os.path.getsize(p):
            rows.append(np.loadtxt(p, ndmin=2))
        os.remove(p)
    a = np.concatenate(rows) if rows else np.zeros((0, 3))
    o = np.lexsort((a[:, 0], a[:, 1]))
    return a[o, 1].astype(np.int32), a[o, 0].astype(np.int32), a[o, 2].astype(np.float64)


def main():
    driver = os.path.abspath(sys.argv[1])
    more = [int(x) for x in sys.argv[2:]]
    for name, seed in CASES.items():
        t = mcl_ref.small_case(seed)  # asserts that every branch fires
        save = dict(m=t["m"], n=t["n"], cp=t["cp"], jc=t["jc"], ir=t["ir"], val=t["val"],
                    params=np.asarray(mcl_ref.PARAM_SETS, np.float64), ranks=np.asarray([1] + more))
        with tempfile.TemporaryDirectory() as tmp:
            mtx = os.path.join(tmp, "in.mtx")
            write_mtx(mtx, t)
            for k, params in enumerate(mcl_ref.PARAM_SETS):
                col, row, val = run_reference(driver, mtx, params, 1, tmp)
                for ranks in more:
                    c2, r2, v2 = run_reference(driver, mtx, params, ranks, tmp)
                    assert np.array_equal(col, c2) and np.array_equal(row, r2)
                    assert np.array_equal(val.view(np.uint64), v2.view(np.uint64)), (name, params, ranks)
                save[f"out{k}_col"], save[f"out{k}_row"], save[f"out{k}_val"] = col, row, val
        np.savez_compressed(os.path.join(HERE, f"mcl_{name}.npz"), **save)
        print(name, "written:", {k: len(save[f"out{k}_col"]) for k in range(len(mcl_ref.PARAM_SETS))})


if __name__ == "__main__":
    main()
