"""Writes tests/golden/betwcent_<case>.npz from the reference's own BetwCent binary.

The binary is Applications/BetwCent.cpp of the reference, compiled unmodified against the
objects that oracle/Makefile builds into oracle/_ref (REF = the reference's root):

    g++ -O2 -fopenmp -DTHREADED -std=c++14 -w -I$REF/include -I$REF/include/CombBLAS \
        -I$REF/psort-1.0/include -I$REF/usort/include -I$REF/graph500-1.2/generator/include \
        -I$MPI_HOME/include $REF/Applications/BetwCent.cpp oracle/_ref/{CommGrid,MPIType,MPIOp,MemoryPool,hash,mmio}.o \
        oracle/_ref/gen_*.o -o betwcent -Wl,-rpath,/usr/lib/x86_64-linux-gnu -Wl,-rpath,$MPI_HOME/lib \
        $MPI_HOME/lib/libmpicxx.so $MPI_HOME/lib/libmpi.so -lm

(the system libstdc++ has to come before MPI_HOME's at run time).  Usage:

    python tests/golden/make_betwcent_golden.py /path/to/betwcent

It runs at ONE rank: `betwcent <dir> K batch out.txt` reads <dir>/input.mtx as AT (so the file
holds the transpose of A: a line "i j" is the edge j -> i), takes the first 2^K vertices whose
column of AT stores something as roots, and writes bc as "index 1 value" lines with 21 significant digits.  None of the
cases has a loop (the reference would put a root with a loop into its own first fringe; the
library drops loops).

Each fixture holds the input (A as COO), the roots handed to the library, the reference's roots
and bc, the exact bc (tests/betwcent_ref.py, fractions) rounded to double, the level sizes per
batch, the largest depth D, the largest degree, the largest path count and the batch size.
The script asserts that the reference agrees with the exact values within
K * 2^-52 * (bc + nroots), K = D * (degree + 4) + nroots + batches + 2, and that the largest path
count is below 2^31 (the reference counts paths in int).

The components case adds the isolated vertex 0 to the library's roots: the reference cannot
take it (its column of AT is empty), and it adds nothing to any bc, which the script asserts
on the exact values."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import betwcent_ref as br  # noqa: E402
import hipmcl_ref as hr  # noqa: E402


def lattice(k=12):
    """k x k grid, edges both ways: C(2k - 2, k - 1) shortest paths between opposite corners"""
    row, col = [], []
    for i in range(k):
        for j in range(k):
            v = i * k + j
            for di, dj in ((0, 1), (1, 0)):
                if i + di < k and j + dj < k:
                    w = (i + di) * k + (j + dj)
                    row += [v, w]
                    col += [w, v]
    return hr.from_coo(k * k, k * k, row, col, np.ones(len(row)))


def rmat():
    z = np.load(os.path.join(HERE, "rmat_s8_ef16_A.npz"))
    return {k: (int(z[k]) if k in ("m", "n") else z[k]) for k in z.files}


def components():
    """0 isolated; {1, 2} a two-vertex component; 3 .. 20 a 3 x 6 grid, both ways; 21 .. 35 a directed
    cycle with chords; 36 .. 47 a star out of 36"""
    e = [(1, 2), (2, 1)]
    for i in range(3):
        for j in range(6):
            v = 3 + i * 6 + j
            if j + 1 < 6:
                e += [(v, v + 1), (v + 1, v)]
            if i + 1 < 3:
                e += [(v, v + 6), (v + 6, v)]
    cyc = list(range(21, 36))
    for x, v in enumerate(cyc):
        e.append((v, cyc[(x + 1) % len(cyc)]))
        if x % 4 == 0:
            e.append((v, cyc[(x + 5) % len(cyc)]))
    e += [(36, v) for v in range(37, 48)]
    row, col = zip(*e)
    return hr.from_coo(48, 48, row, col, np.ones(len(row)))


CASES = {"lattice": (lattice, 3, 4, []), "rmat": (rmat, 3, 4, []), "components": (components, 4, 4, [0])}


def run_reference(binary, t, K, batch):
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "input.mtx"), "w") as f:
            f.write("%%MatrixMarket matrix coordinate pattern general\n")
            f.write(f"{t['n']} {t['n']} {len(t['ir'])}\n")
            for i, j in zip(t["ir"].tolist(), hr.cols_of(t).tolist()):
                f.write(f"{j + 1} {i + 1}\n")  # the file is AT
        out = os.path.join(d, "out.txt")
        env = dict(os.environ, LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:" + os.environ.get("LD_LIBRARY_PATH", ""),
                   OMP_NUM_THREADS="1")
        subprocess.run([binary, d, str(K), str(batch), out], check=True, env=env, stdout=subprocess.DEVNULL)
        lines = open(out).read().split("\n")
    head = lines[0].split()  # "n 1 entries", then "index 1 value" with indices from 1
    assert int(head[0]) == t["n"] and int(head[1]) == 1
    bc = np.zeros(t["n"])
    for ln in lines[1:]:
        if ln.strip():
            i, _, v = ln.split()
            bc[int(i) - 1] = float(v)
    return bc


def main(binary):
    for name, (make, K, batch, extra) in CASES.items():
        t = make()
        assert not np.any(t["ir"] == hr.cols_of(t)), "no loops"
        outdeg = np.bincount(t["ir"], minlength=t["n"])
        ref_roots = np.flatnonzero(outdeg > 0)[:2 ** K]
        assert len(ref_roots) == 2 ** K
        roots = np.array(extra + ref_roots.tolist(), np.int64)
        bc_ref = run_reference(binary, t, K, batch)
        ex_ref = br.brandes(t, ref_roots.tolist(), batch)
        ex = br.brandes(t, roots.tolist(), batch)
        assert ex["bc"] == ex_ref["bc"]  # an isolated root adds nothing
        D, deg = max(ex["depth"]), br.max_degree(t)
        Kb = br.bound_factor(D, deg, len(ref_roots), len(ex_ref["levels"]))
        exact = np.array([float(x) for x in ex["bc"]])
        err = np.abs(bc_ref - exact)
        bound = Kb * 2.0 ** -52 * (exact + len(ref_roots))
        assert np.all(err <= bound), (name, err.max(), bound.min())
        assert ex["sigma_max"] < 2 ** 31
        lv = ex["levels"]
        flat = np.array([x for b in lv for x in b], np.int64)
        np.savez_compressed(os.path.join(HERE, f"betwcent_{name}.npz"), n=np.int64(t["n"]), row=t["ir"].astype(np.int32),
                            col=hr.cols_of(t).astype(np.int32), roots=roots, ref_roots=ref_roots.astype(np.int64),
                            batch=np.int64(batch), bc_ref=bc_ref, bc_exact=exact, level_sizes=flat,
                            level_counts=np.array([len(b) for b in lv], np.int64), depth=np.int64(D),
                            degree=np.int64(deg), sigma_max=np.float64(ex["sigma_max"]))
        print(f"{name}: n {t['n']} nnz {len(t['ir'])} roots {len(roots)} D {D} degree {deg} sigma_max {ex['sigma_max']} "
              f"K {Kb} max |ref - exact| {err.max():.3e} max bc {exact.max():.6g}")


if __name__ == "__main__":
    main(sys.argv[1])
