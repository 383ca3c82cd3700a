"""Writes tests/golden/spmv_<case>.npz and sevenvertex_x.txt / sevenvertex_y.txt from the reference's own
SpMV<PlusTimesSRing<double,double>> and SpMV<MinPlusSRing<double,double>>, run by
tools/ref_spmv_driver.cpp (compile it by the line in its header comment).

    python tests/golden/make_spmv_golden.py <path to ref_spmv_driver>

Every run is made at 1 rank and at 4 ranks (a 2 x 2 grid, launched with /opt/conda/bin/mpirun or
$MPIRUN) with OMP_NUM_THREADS=1.  The script asserts that
  - the 1-rank and the 4-rank outputs are bit-equal for MinPlus and for the `dyadic` case,
  - they are within |y1 - y4| <= 2 (L + 2) 2^-53 sum_j |a(i, j) x[j]| per row for PlusTimes,
  - the restatement (tests/spmv_ref.py) agrees with the reference to the same standard.

A fixture holds inputs and reference outputs only: m, n, the stored entries (row, col) in column-major
order, and per semiring s in (pt, mp): val_<s>, the dense x_<s>, the reference's dense y_<s> (1 rank)
and y4_<s> (4 ranks); per sparse vector k (its entries are x_<s> at the ids xs_<k>): ys_<s>_<k>_ind /
_val and ys4_<s>_<k>_ind / _val.

Cases
  rmat     the pattern of rmat_s10_ef16_A.npz: 1024 x 1024, 10 652 entries, longest row 465, 453 empty
           rows.  PlusTimes: values helpers.random_values_host (U[-1, 1)), x U[-1, 1) from seed 1810.
           MinPlus: both shifted into (0, 1), so no sum is zero; one stored value and one x entry are
           DBL_MAX (inf_plus).  Sparse vectors: the even ids, and 16 ids.
  dyadic   the same pattern, values and x multiples of 2^-10 of magnitude below 1: every sum is exact,
           so the reference's bits are the restatement's on every grid.
  rect     130 x 67 at density 0.2, values and x U[-1, 1): neither extent is a multiple of 64, and a
           2 x 2 grid gets blocks of 65 / 65 rows and 33 / 34 columns.
  sevenvertex  x (dyadic, every entry stored) and the reference's PlusTimes y as the two vector files
           tools/multtest reads."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import helpers  # noqa: E402
import hipmcl_ref as hr  # noqa: E402
import spmv_ref as sv  # noqa: E402

DBL_MAX = sv.DBL_MAX
SEMIRINGS = (("pt", sv.PLUS_TIMES), ("mp", sv.MIN_PLUS))


def coo_of(t):
    return t["ir"].astype(np.int64), hr.cols_of(t)


def write_vector(path, n, ind, val):
    with open(path, "w") as f:
        f.write(f"{n} 1 {len(ind)}\n")
        for i, v in zip(ind.tolist(), val.tolist()):
            f.write(f"{i + 1} 1 {v!r}\n")


def write_matrix(path, m, n, row, col, val):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{m} {n} {len(row)}\n")
        for i, j, v in zip(row.tolist(), col.tolist(), val.tolist()):
            f.write(f"{i + 1} {j + 1} {v!r}\n")


def run_reference(binary, m, n, row, col, val, x, xs, ranks):
    """-> {kind: (ind, val)} for kind in pt_dense, pt_sparse, mp_dense, mp_sparse"""
    with tempfile.TemporaryDirectory() as d:
        mtx, fx, fs, out = (os.path.join(d, k) for k in ("a.mtx", "x.txt", "xs.txt", "out.txt"))
        write_matrix(mtx, m, n, row, col, val)
        write_vector(fx, n, np.arange(n), x)
        write_vector(fs, n, xs, x[xs])
        cmd = [binary, mtx, fx, fs, out]
        if ranks > 1:
            cmd = [os.environ.get("MPIRUN", "/opt/conda/bin/mpirun"), "-n", str(ranks)] + cmd
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS="1",  # the system libstdc++ before the MPI prefix's
                                      LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:" + os.environ.get("LD_LIBRARY_PATH", "")),
                             timeout=600)
        assert run.returncode == 0 and os.path.exists(out), run.stdout[-800:]
        got = {}
        for ln in open(out):
            kind, i, b = ln.split()
            got.setdefault(kind, []).append((int(i), int(b, 16)))
    res = {}
    for kind in ("pt_dense", "pt_sparse", "mp_dense", "mp_sparse"):
        e = got.get(kind, [])
        res[kind] = (np.array([i for i, _ in e], np.int64), np.array([b for _, b in e], np.uint64).view(np.float64))
    for s in ("pt", "mp"):
        assert np.array_equal(res[s + "_dense"][0], np.arange(m))
    return res


def same_bits(a, b):
    return np.array_equal(sv.bits(a), sv.bits(b))


def check_pair(name, what, exact, a, b, bound):
    if exact:
        assert same_bits(a, b), (name, what)
    else:
        assert np.all(np.abs(a - b) <= bound), (name, what, float(np.max(np.abs(a - b) - bound)))


def case_inputs(name):
    """-> m, n, row, col, {s: val}, {s: x}, {k: ids}, exact (every sum exact)"""
    if name in ("rmat", "dyadic"):
        t = helpers.load_npz("rmat_s10_ef16_A.npz")
        row, col = coo_of(t)
        lens = np.bincount(row, minlength=t["m"])
        assert (t["m"], t["n"], len(row), int(lens.max()), int((lens == 0).sum())) == (1024, 1024, 10652, 465, 453)
        n = t["n"]
        rng = np.random.default_rng(1810)
        if name == "rmat":
            v = helpers.random_values_host(t)["val"]
            x = rng.uniform(-1.0, 1.0, n)
            vm, xm = (v + 1.0) * 0.499 + 0.001, (x + 1.0) * 0.499 + 0.001
            assert vm.min() > 0 and xm.min() > 0 and vm.max() < 1 and xm.max() < 1
            hub = int(np.argmax(lens))
            vm[np.flatnonzero(row == hub)[3]] = DBL_MAX
            xm[int(col[np.flatnonzero(row == hub)[7]])] = DBL_MAX
            vals, xs = dict(pt=v, mp=vm), dict(pt=x, mp=xm)
        else:
            v = rng.integers(-700, 900, len(row)).astype(np.float64) / 1024.0
            x = rng.integers(-900, 700, n).astype(np.float64) / 1024.0
            vals, xs = dict(pt=v, mp=v), dict(pt=x, mp=x)
        sparse = dict(even=np.arange(0, n, 2), k16=np.sort(rng.choice(n, 16, replace=False)))
        return t["m"], n, row, col, vals, xs, sparse, name == "dyadic"
    if name == "rect":
        rng = np.random.default_rng(13067)
        m, n = 130, 67
        mask = rng.random((n, m)) < 0.2  # column-major
        col, row = np.nonzero(mask)
        v, x = rng.uniform(-1.0, 1.0, len(row)), rng.uniform(-1.0, 1.0, n)
        sparse = dict(even=np.arange(0, n, 2), k16=np.sort(rng.choice(n, 16, replace=False)))
        return m, n, row.astype(np.int64), col.astype(np.int64), dict(pt=v, mp=v), dict(pt=x, mp=x), sparse, False
    raise ValueError(name)


def make_case(binary, name):
    m, n, row, col, vals, xs, sparse, exact = case_inputs(name)
    out = dict(m=np.int64(m), n=np.int64(n), row=row.astype(np.int32), col=col.astype(np.int32))
    for s, sr in SEMIRINGS:
        t = hr.from_coo(m, n, row, col, vals[s])
        x = xs[s]
        out["val_" + s], out["x_" + s] = vals[s], x
        bound = sv.bound(t, x, pc=2) if sr == sv.PLUS_TIMES else np.zeros(m)
        ex = exact or sr == sv.MIN_PLUS
        for k, ids in sparse.items():
            out["xs_" + k] = ids.astype(np.int64)
            one = run_reference(binary, m, n, row, col, vals[s], x, ids, 1)
            four = run_reference(binary, m, n, row, col, vals[s], x, ids, 4)
            # dense
            check_pair(name, (s, "dense 1 vs 4"), ex, one[s + "_dense"][1], four[s + "_dense"][1], bound)
            for cuts in (None, [n // 2]):
                check_pair(name, (s, "dense ref", cuts), ex, sv.spmv(t, x, sr, cuts), one[s + "_dense"][1], bound)
            out["y_" + s], out["y4_" + s] = one[s + "_dense"][1], four[s + "_dense"][1]
            # sparse: the bound over the columns that take part
            sub = np.isin(col, ids)
            ts = hr.from_coo(m, n, row[sub], col[sub], vals[s][sub])
            sb = sv.bound(ts, x, pc=2) if sr == sv.PLUS_TIMES else np.zeros(m)
            i1, v1 = one[s + "_sparse"]
            i4, v4 = four[s + "_sparse"]
            assert np.array_equal(i1, i4), (name, s, k)
            check_pair(name, (s, k, "sparse 1 vs 4"), ex, v1, v4, sb[i1])
            for cuts in (None, [n // 2]):
                ri, rv = sv.spmspv(t, ids, x[ids], sr, cuts)
                assert np.array_equal(ri, i1), (name, s, k, cuts)
                check_pair(name, (s, k, "sparse ref", cuts), ex, rv, v1, sb[i1])
            out[f"ys_{s}_{k}_ind"], out[f"ys_{s}_{k}_val"] = i1, v1
            out[f"ys4_{s}_{k}_ind"], out[f"ys4_{s}_{k}_val"] = i4, v4
            print(f"{name} {s} {k}: dense rows {m}, sparse entries {len(i1)}, exact {ex}, "
                  f"max |y1 - y4| {float(np.max(np.abs(one[s + '_dense'][1] - four[s + '_dense'][1]))):.3g}")
    np.savez_compressed(os.path.join(HERE, f"spmv_{name}.npz"), **out)


def make_sevenvertex(binary):
    t = helpers.load_npz("sevenvertex_A.npz")
    row, col = coo_of(t)
    x = np.array([0.5, -1.25, 2.0, 0.75, -0.5, 1.5, 3.0])
    assert t["n"] == len(x)
    one = run_reference(binary, t["m"], t["n"], row, col, t["val"], x, np.arange(t["n"]), 1)
    four = run_reference(binary, t["m"], t["n"], row, col, t["val"], x, np.arange(t["n"]), 4)
    yi, yv = one["pt_sparse"]
    assert same_bits(one["pt_dense"][1], four["pt_dense"][1]) and same_bits(yv, four["pt_sparse"][1])
    assert same_bits(one["pt_dense"][1], sv.spmv(t, x)) and same_bits(yv, sv.spmspv(t, np.arange(t["n"]), x)[1])
    dense = one["pt_dense"][1]
    assert np.array_equal(dense[yi], yv) and np.all(np.delete(dense, yi) == 0.0)
    write_vector(os.path.join(HERE, "sevenvertex_x.txt"), t["n"], np.arange(t["n"]), x)
    write_vector(os.path.join(HERE, "sevenvertex_y.txt"), t["m"], yi, yv)
    print("sevenvertex: y", dense.tolist())


def main(binary):
    for name in ("rmat", "dyadic", "rect"):
        make_case(binary, name)
    make_sevenvertex(binary)


if __name__ == "__main__":
    main(sys.argv[1])
