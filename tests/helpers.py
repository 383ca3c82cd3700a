"""Shared test helpers: golden fixtures, digests and the CPU oracle (ctypes).

The oracle (oracle/liboracle.so) is TEST INFRASTRUCTURE: it is only ever used
here as the checker (and by smoke()/bench.py's cpu_baseline).
"""
import ctypes
import json
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
ORACLE_SO = os.path.join(REPO, "oracle", "liboracle.so")


# --------------------------------------------------------------------------
# tiles as plain dicts of numpy arrays (DCSC: cp int64, jc/ir int32, val f64)
# --------------------------------------------------------------------------
def load_npz(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    return dict(m=int(z["m"]), n=int(z["n"]), cp=z["cp"].astype(np.int64), jc=z["jc"].astype(np.int32),
                ir=z["ir"].astype(np.int32), val=z["val"].astype(np.float64))


def golden():
    with open(os.path.join(GOLDEN, "golden.json")) as f:
        return json.load(f)


def _mix64(z):
    z = z.astype(np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def tile_cols(t):
    """expanded column index per nonzero"""
    cnt = np.diff(t["cp"])
    return np.repeat(t["jc"].astype(np.int64), cnt)


def digest(t, roff=0, coff=0):
    """Same digest as oracle/ref_driver.cpp tile_digest (tests/golden/make_golden.py)."""
    col = tile_cols(t) + coff
    row = t["ir"].astype(np.int64) + roff
    h = _mix64((col.astype(np.uint64) << np.uint64(32)) | row.astype(np.uint64))
    vb = _mix64(np.ascontiguousarray(t["val"], dtype=np.float64).view(np.uint64))
    with np.errstate(over="ignore"):
        hs = int(np.sum(h, dtype=np.uint64))
        hv = int(np.sum(h * vb, dtype=np.uint64))
    unsorted = 0
    if len(t["jc"]) > 1:
        unsorted += int(np.sum(np.diff(t["jc"].astype(np.int64)) <= 0))
    if len(row) > 1:
        d = np.diff(t["ir"].astype(np.int64))
        same = np.diff(col) == 0
        unsorted += int(np.sum((d <= 0) & same))
    return dict(nnz=int(len(t["ir"])), nzc=int(len(t["jc"])), hs="%016x" % hs, hv="%016x" % hv,
                vsum=float(np.sum(t["val"])), unsorted=unsorted)


def assert_digest_eq(d, g, values=True, vtol=0.0):
    assert d["nnz"] == g["nnz"], (d, g)
    assert d["hs"] == g["hs"], (d, g)
    assert d["unsorted"] == 0
    if values:
        if vtol == 0.0:
            assert d["hv"] == g["hv"], (d, g)
        assert abs(d["vsum"] - g["vsum"]) <= vtol * max(1.0, abs(g["vsum"])), (d, g)


def assert_tiles_bits_equal(c, r):
    """m, n, cp, jc, ir exactly equal; NaN at the same positions (sign and payload of a
    NaN differ between the host and the GPU, so NaN is compared by position only);
    everywhere else the 64 value bits equal: -0.0 != +0.0, unlike assert_tiles_equal."""
    assert c["m"] == r["m"] and c["n"] == r["n"], ((c["m"], c["n"]), (r["m"], r["n"]))
    np.testing.assert_array_equal(np.asarray(c["cp"], np.int64), np.asarray(r["cp"], np.int64))
    np.testing.assert_array_equal(np.asarray(c["jc"]), np.asarray(r["jc"]))
    np.testing.assert_array_equal(np.asarray(c["ir"]), np.asarray(r["ir"]))
    cv = np.ascontiguousarray(c["val"], dtype=np.float64)
    rv = np.ascontiguousarray(r["val"], dtype=np.float64)
    cn, rn = np.isnan(cv), np.isnan(rv)
    bad = (cn != rn) | (~cn & ~rn & (cv.view(np.uint64) != rv.view(np.uint64)))
    if bad.any():
        at = np.flatnonzero(bad)
        cols = tile_cols(r)
        first = [(int(cols[i]), int(r["ir"][i]), "%016x" % int(cv.view(np.uint64)[i]),
                  "%016x" % int(rv.view(np.uint64)[i])) for i in at[:8]]
        raise AssertionError(f"{len(at)} of {len(rv)} values differ in their bits; "
                             f"first (col, row, got bits, want bits): {first}")


def assert_tiles_equal(c, r, rtol=0.0, bound=None):
    """Indices bit-exact; values exact (rtol=0) or |dc| <= rtol * bound (elementwise)."""
    assert c["m"] == r["m"] and c["n"] == r["n"]
    np.testing.assert_array_equal(np.asarray(c["cp"], np.int64), np.asarray(r["cp"], np.int64))
    np.testing.assert_array_equal(np.asarray(c["jc"]), np.asarray(r["jc"]))
    np.testing.assert_array_equal(np.asarray(c["ir"]), np.asarray(r["ir"]))
    if rtol == 0.0:
        np.testing.assert_array_equal(np.asarray(c["val"]), np.asarray(r["val"]))
    else:
        b = np.abs(r["val"]) if bound is None else bound
        err = np.abs(np.asarray(c["val"]) - np.asarray(r["val"]))
        bad = err > rtol * b + 1e-300
        assert not bad.any(), f"{bad.sum()} values off, max rel {float(np.max(err / (b + 1e-300)))}"


# --------------------------------------------------------------------------
# oracle (ctypes)
# --------------------------------------------------------------------------
class OTile(ctypes.Structure):
    _fields_ = [("m", ctypes.c_int64), ("n", ctypes.c_int64), ("nnz", ctypes.c_int64), ("nzc", ctypes.c_int64),
                ("cp", ctypes.POINTER(ctypes.c_int64)), ("jc", ctypes.POINTER(ctypes.c_int32)),
                ("ir", ctypes.POINTER(ctypes.c_int32)), ("val", ctypes.POINTER(ctypes.c_double))]


_lib = None


def oracle():
    global _lib
    if _lib is None:
        if not os.path.exists(ORACLE_SO):
            import subprocess
            subprocess.run(["make", "-C", os.path.join(REPO, "oracle")], check=True, capture_output=True)
        _lib = ctypes.CDLL(ORACLE_SO)
        P = ctypes.POINTER(OTile)
        _lib.ocbg_rmat_tile.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, P]
        _lib.ocbg_local_hybrid.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P]
        _lib.ocbg_local_heap.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P]
        _lib.ocbg_summa.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
        _lib.ocbg_symbolic.argtypes = [P, P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                       ctypes.c_int]
        _lib.ocbg_rmat_edges.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        _lib.ocbg_free.argtypes = [P]
    return _lib


def _to_otile(t):
    keep = dict(cp=np.ascontiguousarray(t["cp"], np.int64), jc=np.ascontiguousarray(t["jc"], np.int32),
                ir=np.ascontiguousarray(t["ir"], np.int32), val=np.ascontiguousarray(t["val"], np.float64))
    o = OTile(t["m"], t["n"], len(keep["ir"]), len(keep["jc"]),
              keep["cp"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
              keep["jc"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
              keep["ir"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
              keep["val"].ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return o, keep


def _from_otile(o):
    lib = oracle()
    t = dict(m=o.m, n=o.n,
             cp=np.ctypeslib.as_array(o.cp, (o.nzc + 1,)).copy(),
             jc=np.ctypeslib.as_array(o.jc, (max(o.nzc, 1),))[:o.nzc].copy(),
             ir=np.ctypeslib.as_array(o.ir, (max(o.nnz, 1),))[:o.nnz].copy(),
             val=np.ctypeslib.as_array(o.val, (max(o.nnz, 1),))[:o.nnz].copy())
    lib.ocbg_free(ctypes.byref(o))
    return t


SR = {"plus": 0, "plus_times": 0, "minplus": 1, "min_plus": 1}


def oracle_rmat(scale, ef=16, seed=0xDECAFBAD, nthreads=0):
    o = OTile()
    oracle().ocbg_rmat_tile(scale, ef, seed, nthreads, ctypes.byref(o))
    return _from_otile(o)


def oracle_edges(scale, e0, e1, seed=0xDECAFBAD):
    s = np.empty(e1 - e0, np.int64)
    d = np.empty(e1 - e0, np.int64)
    oracle().ocbg_rmat_edges(scale, e0, e1, seed, s.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                             d.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return s, d


def oracle_local(A, B, sr="plus", heap=False, nthreads=0):
    a, ka = _to_otile(A)
    b, kb = _to_otile(B)
    c = OTile()
    f = oracle().ocbg_local_heap if heap else oracle().ocbg_local_hybrid
    rc = f(ctypes.byref(a), ctypes.byref(b), SR[sr], nthreads, ctypes.byref(c))
    assert rc == 0
    return _from_otile(c)


def oracle_summa(A, B, pr, algo="doublebuff", sr="plus", nthreads=0):
    a, ka = _to_otile(A)
    b, kb = _to_otile(B)
    c = OTile()
    rc = oracle().ocbg_summa(ctypes.byref(a), ctypes.byref(b), pr, 0 if algo == "doublebuff" else 1, SR[sr],
                             nthreads, ctypes.byref(c))
    assert rc == 0, rc
    return _from_otile(c)


def oracle_symbolic(A, B, nthreads=0):
    a, ka = _to_otile(A)
    b, kb = _to_otile(B)
    nz = len(B["jc"])
    f = np.zeros(max(nz, 1), np.int64)
    n = np.zeros(max(nz, 1), np.int64)
    oracle().ocbg_symbolic(ctypes.byref(a), ctypes.byref(b), f.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                           n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nthreads)
    return f[:nz], n[:nz]


def abs_tile(t):
    u = dict(t)
    u["val"] = np.abs(t["val"])
    return u


# ---- Galerkin path host restatements (checkers) ----
_M64 = (1 << 64) - 1


def _mix_np(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


POISSON1_CDF = np.array([0.36787944117144233, 0.7357588823428847, 0.9196986029286058, 0.9810118431238463,
                         0.9963401531726563, 0.9994058151824183, 0.999916758850712, 0.9999897508033253,
                         0.999998874797402, 0.9999998885745216, 0.9999999899522336, 0.9999999991683892])


def restriction_host(scale, order=2, seed=0x5EED):
    """global restriction operator of cbg_restriction_tile (csrc/cbg_ops.hip k_restrict_count /
    k_restrict_fill): genrestrict.m:11's sprand(n, n/order, order/n) shape -- Poisson(1)
    nonzeros per fine row (count by inversion of the CDF table), uniform coarse columns,
    values in (0, 1], a column drawn twice in one row summed."""
    n = 1 << scale
    nc = n // order
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _mix_np(np.uint64(seed) ^ (i * np.uint64(0xD1B54A32D192ED03)))
        u = (_mix_np(h ^ np.uint64(0x5851F42D4C957F2D)) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        k = np.searchsorted(POISSON1_CDF, u, side="right")
        rows = np.repeat(np.arange(n, dtype=np.int64), k)
        starts = np.repeat(np.cumsum(k) - k, k)
        j = np.arange(len(rows), dtype=np.int64) - starts
        hj = _mix_np(h[rows] + (j + 1).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    cols = (hj % np.uint64(nc)).astype(np.int64)
    vals = ((_mix_np(hj) >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * (1.0 / 9007199254740992.0)
    o = np.lexsort((j, rows, cols))
    r, c, v = rows[o], cols[o], vals[o]
    head = np.ones(len(r), bool)
    head[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    run = np.cumsum(head) - 1
    uv = np.zeros(int(head.sum()))
    np.add.at(uv, run, v)  # duplicates summed in draw order
    ur, uc = r[head], c[head]
    jc, start = np.unique(uc, return_index=True)
    return dict(m=n, n=nc, cp=np.append(start, len(ur)).astype(np.int64), jc=jc.astype(np.int32),
                ir=ur.astype(np.int32), val=uv)


def random_values_host(t, seed=0x5EEDF00D, roff=0, coff=0):
    """Tile.set_random_values (csrc/cbg_ops.hip random_value) on a host tile: a copy with
    every (row, col) value = U[-1, 1) from mix(((col << 32) | row) ^ seed * K)."""
    col = tile_cols(t).astype(np.uint64) + np.uint64(coff)
    row = t["ir"].astype(np.uint64) + np.uint64(roff)
    with np.errstate(over="ignore"):
        z = _mix_np(((col << np.uint64(32)) | row) ^ (np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)))
    u = dict(t)
    u["val"] = (z >> np.uint64(11)).astype(np.float64) * (1.0 / 4503599627370496.0) - 1.0
    return u


def transpose_host(d):
    cols = np.repeat(d["jc"].astype(np.int64), np.diff(d["cp"]))
    rows = d["ir"].astype(np.int64)
    o = np.lexsort((cols, rows))
    r, c, v = rows[o], cols[o], d["val"][o]
    jc, start = np.unique(r, return_index=True)
    return dict(m=d["n"], n=d["m"], cp=np.append(start, len(r)).astype(np.int64), jc=jc.astype(np.int32),
                ir=c.astype(np.int32), val=v)


def add_diag_host(d, dv):
    """d + diag(dv) for a host DCSC dict with no diagonal entries (loops removed)."""
    n = len(dv)
    cols = np.concatenate([np.repeat(d["jc"].astype(np.int64), np.diff(d["cp"])), np.arange(n)])
    rows = np.concatenate([d["ir"].astype(np.int64), np.arange(n)])
    vals = np.concatenate([d["val"], dv])
    o = np.lexsort((rows, cols))
    r, c, v = rows[o], cols[o], vals[o]
    jc, start = np.unique(c, return_index=True)
    return dict(m=d["m"], n=d["n"], cp=np.append(start, len(r)).astype(np.int64), jc=jc.astype(np.int32),
                ir=r.astype(np.int32), val=v)


def dcsc_from_cols(m, n, cols, val=None):
    """DCSC dict from a list of row arrays (one per column, each ascending; empty
    columns are dropped); values 1.0 unless given (flat, in column order)"""
    cnt = np.array([len(c) for c in cols], np.int64)
    jc = np.flatnonzero(cnt > 0)
    ir = np.concatenate([np.asarray(c, np.int64) for c in cols] + [np.zeros(0, np.int64)])
    return dict(m=int(m), n=int(n), cp=np.concatenate([[0], np.cumsum(cnt[jc])]).astype(np.int64),
                jc=jc.astype(np.int32), ir=ir.astype(np.int32),
                val=np.ones(len(ir)) if val is None else np.asarray(val, np.float64))


def split_cols_host(d, cut):
    """Tile.split_cols on a host tile: columns [0, cut) and [cut, n) renumbered from 0"""
    k = int(np.searchsorted(d["jc"], cut))
    e = int(d["cp"][k])
    left = dict(m=d["m"], n=cut, cp=d["cp"][:k + 1].copy(), jc=d["jc"][:k].copy(), ir=d["ir"][:e].copy(),
                val=d["val"][:e].copy())
    right = dict(m=d["m"], n=d["n"] - cut, cp=d["cp"][k:] - e, jc=(d["jc"][k:] - cut).astype(np.int32),
                 ir=d["ir"][e:].copy(), val=d["val"][e:].copy())
    return left, right


def split_rows_host(d, cut):
    """Tile.split_rows on a host tile: rows [0, cut) and [cut, m) renumbered from 0"""
    cols = tile_cols(d)
    out = []
    for keep, off, mm in ((d["ir"] < cut, 0, cut), (d["ir"] >= cut, cut, d["m"] - cut)):
        c = cols[keep]
        jc, start = np.unique(c, return_index=True)
        out.append(dict(m=mm, n=d["n"], cp=np.append(start, len(c)).astype(np.int64), jc=jc.astype(np.int32),
                        ir=(d["ir"][keep] - off).astype(np.int32), val=d["val"][keep].copy()))
    return out[0], out[1]


def concat_cols_host(parts):
    """Tile.concat_cols on host tiles of equal m: columns laid side by side"""
    off = np.concatenate([[0], np.cumsum([p["n"] for p in parts])])
    eoff = np.concatenate([[0], np.cumsum([len(p["ir"]) for p in parts])])
    return dict(m=parts[0]["m"], n=int(off[-1]),
                cp=np.concatenate([[0]] + [p["cp"][1:] + e for p, e in zip(parts, eoff)]).astype(np.int64),
                jc=np.concatenate([p["jc"].astype(np.int64) + o for p, o in zip(parts, off)]).astype(np.int32),
                ir=np.concatenate([p["ir"] for p in parts]).astype(np.int32),
                val=np.concatenate([p["val"] for p in parts]))


# --------------------------------------------------------------------------
# operand builders shared by the GPU tests (tests/test_gpu_local.py and
# tests/test_gpu_value_bits.py); each draws from its own seeded generator
# --------------------------------------------------------------------------
def rand_tile(rng, m, n, density, lo=-1.0, hi=1.0, hub_cols=()):
    M = (rng.random((m, n)) < density)
    for c in hub_cols:
        M[:, c] = rng.random(m) < 0.8
    vals = rng.uniform(lo, hi, size=(m, n))
    cols, rows = np.nonzero(M.T)
    jc, start = np.unique(cols, return_index=True)
    return dict(m=m, n=n, cp=np.append(start, len(rows)).astype(np.int64), jc=jc.astype(np.int32),
                ir=rows.astype(np.int32), val=vals[rows, cols].astype(np.float64))


def rand_hub_operands(seed=0):
    """hub columns in A and B force the wave, block and big-column (slab) paths"""
    rng = np.random.default_rng(seed)
    Ah = rand_tile(rng, 3000, 2500, 0.004, hub_cols=(3, 77))
    Bh = rand_tile(rng, 2500, 1800, 0.01, hub_cols=(5,))
    return Ah, Bh


def sparse_cols(rng, m, lens, dup_rows=None):
    """DCSC with column j holding lens[j] distinct sorted random rows (0 = empty column dropped)"""
    cols, rows = [], []
    for j, L in enumerate(lens):
        if L == 0:
            continue
        r = np.sort(rng.choice(m if dup_rows is None else dup_rows, L, replace=False))
        cols.append(np.full(L, j))
        rows.append(r)
    cols = np.concatenate(cols)
    rows = np.concatenate(rows)
    jc, start = np.unique(cols, return_index=True)
    return dict(m=m, n=len(lens), cp=np.append(start, len(rows)).astype(np.int64), jc=jc.astype(np.int32),
                ir=rows.astype(np.int32), val=rng.uniform(-1.0, 1.0, len(rows)))


def esc_operands(m):
    """columns of <= 512 products (the expand-sort-compress waves): rows concentrated
    on few values force duplicate keys inside a wave, B columns of many entries on
    empty A columns force several staging rounds"""
    rng = np.random.default_rng(5)
    k = 400
    hot = np.arange(0, m, max(1, m // 40))[:40]      # 40 row values: many duplicates
    lensA = rng.integers(0, 9, k)
    lensA[::7] = 0                                      # empty A columns
    Ah = sparse_cols(rng, m, lensA, dup_rows=hot)
    Ah["n"] = k
    nB = 3000
    ir, cp = [], [0]
    for j in range(nB):
        target = int(rng.choice([1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 100, 128, 160, 200, 256, 300, 400, 512]))
        ks, f = [], 0
        for kk in rng.permutation(k):
            L = int(lensA[kk])
            if f + L > target:
                continue
            ks.append(kk)
            f += L
            if f == target or len(ks) > 200:
                break
        ks = sorted(ks) if ks else [int(np.argmax(lensA == 0))]
        ir.extend(ks)
        cp.append(len(ir))
    Bh = dict(m=k, n=nB, cp=np.array(cp, np.int64), jc=np.arange(nB, dtype=np.int32),
              ir=np.array(ir, np.int32), val=rng.uniform(-1.0, 1.0, len(ir)))
    return Ah, Bh


def thin_operands():
    """long B columns over A columns of ONE nonzero (flops per B entry 1 < R / 4: the
    thin-column pass); A's rows come from a small pool so that products collide; a few
    ordinary big and small columns too"""
    rng = np.random.default_rng(21)
    m, k = (1 << 20) + 37, 120000
    pool = rng.choice(m, 30000, replace=False)
    rowsA = rng.choice(pool, k)
    Ah = dict(m=m, n=k, cp=np.arange(k + 1, dtype=np.int64), jc=np.arange(k, dtype=np.int32),
              ir=rowsA.astype(np.int32), val=rng.uniform(0.5, 2.0, k))
    hub = np.sort(rng.choice(m, 20000, replace=False))          # one long A column: a regular big column
    Ah = dict(m=m, n=k + 1, cp=np.append(Ah["cp"], k + len(hub)).astype(np.int64),
              jc=np.arange(k + 1, dtype=np.int32), ir=np.concatenate([Ah["ir"], hub]).astype(np.int32),
              val=np.concatenate([Ah["val"], rng.uniform(0.5, 2.0, len(hub))]))
    lens = list(rng.integers(4100, 30000, 24)) + list(rng.integers(1, 40, 200))
    ir, cp = [], [0]
    for L in lens:
        ir.extend(np.sort(rng.choice(k, int(L), replace=False)))
        cp.append(len(ir))
    ir.extend([0, k])  # the hub column and one short one: a regular big column (one entry alone is a copy)
    cp.append(len(ir))
    nB = len(cp) - 1
    Bh = dict(m=k + 1, n=nB, cp=np.array(cp, np.int64), jc=np.arange(nB, dtype=np.int32),
              ir=np.array(ir, np.int32), val=rng.uniform(-1.0, 1.0, len(ir)))
    return Ah, Bh


def single_entry_operands():
    """B columns with one entry (scaled copies of an A column): short and hub A columns
    (above the 4096-flop big threshold), zero and negative B values, next to ordinary
    small and big columns"""
    rng = np.random.default_rng(5)
    m, k = (1 << 19) + 11, 3000
    lens = np.concatenate([rng.integers(0, 30, k - 6), [5000, 9000, 20000, 70000, 4096, 4097]]).astype(np.int64)
    ir, cp = [], [0]
    for L in lens:
        ir.extend(np.sort(rng.choice(m, int(L), replace=False)))
        cp.append(len(ir))
    Ah = dict(m=m, n=k, cp=np.array(cp, np.int64), jc=np.arange(k, dtype=np.int32), ir=np.array(ir, np.int32),
              val=rng.uniform(-2.0, 2.0, len(ir)))
    bcols = []
    for j in range(400):
        t = j % 4
        if t == 0:    # one entry: a short A column
            bcols.append([int(rng.integers(0, k - 6))])
        elif t == 1:  # one entry: a hub
            bcols.append([int(k - 6 + rng.integers(0, 6))])
        elif t == 2:  # a few short ones
            bcols.append(sorted(rng.choice(k - 6, 5, replace=False).tolist()))
        else:         # hubs and short ones: a big column
            bcols.append(sorted(set(rng.choice(k - 6, 3, replace=False).tolist() + [k - 3, k - 2])))
    cpB = np.cumsum([0] + [len(c) for c in bcols]).astype(np.int64)
    irB = np.concatenate([np.array(c, np.int32) for c in bcols])
    valB = rng.uniform(-1.0, 1.0, len(irB))
    valB[::7] = 0.0  # explicit zero products stay structural entries
    Bh = dict(m=k, n=len(bcols), cp=cpB, jc=np.arange(len(bcols), dtype=np.int32), ir=irB, val=valB)
    return Ah, Bh


def panel_group_operands(m=(1 << 20) + 77):
    """Tall A (m = 2^20 + 77: 5 row panels of 2^18, the last one partial) and a B whose
    columns land in every big-column class: panel groups of 4 and 2 (expected products
    per group <= 4096), single-panel hash pairs, bitmap pairs, a group with > 512 B
    entries, and groups whose products crowd into one panel (nnz > one hash slab), which
    must fall back to per-panel slabs."""
    rng = np.random.default_rng(11)
    heavy, light, local = 3000, 1000, 200  # A columns: 100 rows anywhere / 8 rows / 100 rows in panel 0

    def col(nr, hi):
        return np.sort(rng.choice(hi, nr, replace=False))

    acols = [col(100, m) for _ in range(heavy)] + [col(8, m) for _ in range(light)] + \
            [col(100, 1 << 18) for _ in range(local)]
    k = len(acols)
    cnt = np.array([len(c) for c in acols])
    Ah = dict(m=m, n=k, cp=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), jc=np.arange(k, dtype=np.int32),
              ir=np.concatenate(acols).astype(np.int32),
              val=rng.integers(1, 5, int(cnt.sum())).astype(np.float64))
    groups = [(100, 5, 40, 0), (100, 44, 48, 0), (100, 78, 84, 0), (50, 140, 160, 0), (30, 280, 320, 0),
              (20, 600, 601, 1), (20, 45, 46, 2)]
    bcols = []
    for num, lo, hi, kind in groups:
        for _ in range(num):
            nb = int(rng.integers(lo, hi))
            if kind == 0:
                bcols.append(np.sort(rng.choice(heavy, nb, replace=False)))
            elif kind == 1:
                bcols.append(np.sort(heavy + rng.choice(light, nb, replace=False)))
            else:
                bcols.append(np.sort(heavy + light + rng.choice(local, nb, replace=False)))
    n = len(bcols)
    perm = rng.permutation(n)
    bcols = [bcols[i] for i in perm]
    bc = np.array([len(c) for c in bcols])
    Bh = dict(m=k, n=n, cp=np.concatenate([[0], np.cumsum(bc)]).astype(np.int64), jc=np.arange(n, dtype=np.int32),
              ir=np.concatenate(bcols).astype(np.int32), val=rng.integers(1, 3, int(bc.sum())).astype(np.float64))
    return Ah, Bh


# --------------------------------------------------------------------------
# value palettes with order-independent results (tests/test_gpu_value_bits.py)
#
# A's value depends on the row class ir % ncls, so every C entry combines products of
# ONE class; B's values are small dyadics.  Plus-times: every sum is then exact, or
# inf / NaN whatever the order, and a sum of zeros is -0.0 exactly when every product
# is -0.0.  Min-plus: no -0.0 in B and no -inf, so no +-0 ties and no NaN.
# --------------------------------------------------------------------------
DBL_MAX = float(np.finfo(np.float64).max)
INF = float("inf")
_B_PLUS = [1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 0.0, -0.0]
_B_INT = [1.0, -1.0, 2.0, -2.0]
_ZEROS, _ZEROS1, _INFS = [0.0, -0.0], [0.0, -0.0, 1.0], [INF, -INF, 1.0]
_DY32, _SUB32 = [0.25, -2.25, 3.0, 1024.125, -1.0], [2.0 ** -140, -3 * 2.0 ** -141]
_DY64, _SUB64, _BIG64 = [0.25, -2.25, 3.0], [2.0 ** -1060, 3 * 2.0 ** -1062], [2.0 ** 1000, -3 * 2.0 ** 999]
# class mix: one class in ten holds the infinities, so that NaN stays below 10 % of
# nnz(C) also where many products meet in one entry (the ESC operands' 40 hot rows)
PALETTES = {
    # every A value an exact f32 (the slab kernels' f32 records); f32 subnormals
    "f32": dict(sr="plus", B=_B_PLUS, zeros=True,
                A=[_ZEROS, _DY32, _INFS, _SUB32, _ZEROS1, _DY32, _SUB32, _ZEROS1, _ZEROS, _DY32]),
    # A not f32-exact (f64 records): f64 subnormals, magnitudes outside f32's range
    "f64": dict(sr="plus", B=_B_PLUS, zeros=True,
                A=[_ZEROS, _DY64, _INFS, _SUB64, _BIG64, [2.0 ** -140], _DY64, _SUB64, _BIG64, _ZEROS]),
    # integer-shaped, with explicit +0.0 (0.0 * -1 = -0.0, which int32 cannot carry)
    "int0": dict(sr="both", B=_B_INT, zeros=True,
                 A=[[0.0], [0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0], [1.0, -1.0, 2.0, -2.0, 3.0, -3.0]]),
    # integers without zeros: exact int32 accumulation must stay on
    "int": dict(sr="both", B=_B_INT, zeros=False, A=[[1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0]]),
    # min-plus: the DBL_MAX sentinel of inf_plus, +inf (the empty-slot value), overflow
    "minplus": dict(sr="minplus", B=[1.0, -1.0, 2.0, 0.5, 0.0, DBL_MAX, INF], zeros=False,
                    A=[[0.0, 1.0, -2.25], [INF, 5.0], [DBL_MAX, 3.0], [-DBL_MAX, 2.0], [1.5 * 2.0 ** 1023, 1.0]]),
}


def row_class(ir, ncls):
    """class of a row: a function of the row alone.  The row is scrambled first: a plain
    ir % ncls puts rows on a regular stride (the ESC operands' 40 hot rows are the
    multiples of 125) all in one class."""
    return ((np.asarray(ir, np.int64) * 2654435761) >> 16) % ncls


def with_palette(Ah, Bh, palette, rng):
    """copies of Ah, Bh with the same structure and the palette's values"""
    p = PALETTES[palette] if isinstance(palette, str) else palette
    ncls = len(p["A"])
    w = max(len(c) for c in p["A"])
    table = np.array([[c[i % len(c)] for i in range(w)] for c in p["A"]], np.float64)
    cls = row_class(Ah["ir"], ncls)
    pick = rng.integers(0, 1 << 30, len(cls)) % np.array([len(c) for c in p["A"]])[cls]
    A, B = dict(Ah), dict(Bh)
    A["val"] = table[cls, pick]
    B["val"] = np.array(p["B"], np.float64)[rng.integers(0, len(p["B"]), len(Bh["ir"]))]
    return A, B


def special_shares(C):
    """(NaN share, -0.0 share) of a tile's entries"""
    v = np.asarray(C["val"], np.float64)
    n = max(len(v), 1)
    return float(np.isnan(v).sum()) / n, float(((v == 0.0) & np.signbit(v)).sum()) / n


def assert_palette_not_vacuous(C, palette):
    """on the ORACLE's C: NaN entries < 10 % (the rest is compared bit by bit), and for
    the plus-times palettes that hold zeros -0.0 entries >= 1 %"""
    nan, negz = special_shares(C)
    assert len(C["ir"]) > 0
    assert nan < 0.10, (palette, nan)
    if PALETTES[palette]["zeros"]:
        assert negz >= 0.01, (palette, negz)
    return nan, negz


# --------------------------------------------------------------------------
# bin-boundary and panel-boundary operands (tests/test_gpu_value_bits.py)
# --------------------------------------------------------------------------
SYM_THR = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]   # csrc/cbg_local.hip kSymThr (flops)
NUM_THR = [32, 64, 128, 256, 512, 1024, 2048, 4096]               # kNumThr (exact nnz)
BIG_FLOPS = 4096
PANEL = 1 << 18
NUNIT, NSEVEN = 4200, 600


def boundary_pairs(big=BIG_FLOPS):
    """the (flops, nnz) of the sweep's B columns: every kSymThr t at f = t-1, t, t+1 with a
    full table (z = f) and z = ceil(f / 2); every kNumThr t at z = t-1, t, t+1 with
    f = min(2z, big) (z > big: f = z, necessarily a big column)"""
    pairs = []
    for t in SYM_THR:
        for f in (t - 1, t, t + 1):
            pairs += [(f, f), (f, (f + 1) // 2)]
    for t in NUM_THR:
        for z in (t - 1, t, t + 1):
            pairs.append((max(z, min(2 * z, big)), z))
    return sorted(set(pairs))


def boundary_rows(m, layout, rng):
    """NUNIT distinct rows P (position u = the row of unit column u)"""
    if layout == "dense":       # m = 5000: nearly every row taken
        return rng.permutation(m)[:NUNIT]
    if layout == "random":
        return rng.choice(m, NUNIT, replace=False)
    if layout == "stride128":   # low 7 bits zero: the worst case of a multiplicative hash
        return rng.permutation(m // 128)[:NUNIT] * 128
    if layout == "edges":       # packed around the panel edges and the last row
        edges = [p * PANEL for p in range(1, (m + PANEL - 1) // PANEL)] + [m]
        per = 2 * NUNIT // len(edges)
        near = np.concatenate([np.arange(e - per // 2, e + per // 2) for e in edges])
        must = panel_edge_rows(m)  # the edge rows themselves, always
        near = np.setdiff1d(near[(near >= 0) & (near < m)], must)
        # the edge rows first: the columns of few units hold them too
        return np.concatenate([rng.permutation(must), rng.permutation(near)[:NUNIT - len(must)]])
    raise KeyError(layout)


def boundary_operands(m, layout, sr="plus", mixed=False, pairs=None, seed=3):
    """A: unit columns u = 0..NUNIT-1 holding the single row P[u], twin columns NUNIT+u
    holding the same row with another value; mixed: also NSEVEN columns of the 7 rows
    P[7i..7i+6] and their NSEVEN twins.  B: for each pair (f, z), z <= f <= 2z, a column
    of units 0..z-1 and twins 0..f-z-1 (mixed: as many 7-row columns as fit, units for
    the rest), so that its flops are f and its nnz is z; every pair three times with
    other values.  Every C entry is one product or the sum (min) of two, so it is
    exact in any order.  Returns (Ah, Bh, table) with table[j] = (f, z) of B column j."""
    rng = np.random.default_rng(seed)
    P = boundary_rows(m, layout, rng).astype(np.int64)
    assert len(np.unique(P)) == NUNIT and P.min() >= 0 and P.max() < m
    acols = [[r] for r in P] + [[r] for r in P]
    if mixed:
        sev = [np.sort(P[7 * i:7 * i + 7]) for i in range(NSEVEN)]
        acols += sev + sev
    if sr == "plus":
        av = [0.25, -2.25, 3.0, -1.0, 1024.125, 0.0, -0.0, 2.0 ** -1060, 2.0 ** 1000]
        bv = _B_PLUS
    else:  # no -0.0: a tie between +0.0 and -0.0 has no order-independent minimum
        av = [0.0, 1.0, -2.25, 5.0, 3.0, DBL_MAX, -DBL_MAX, INF, 1.5 * 2.0 ** 1023]
        bv = [1.0, -1.0, 2.0, 0.5, 0.0, DBL_MAX, INF]
    na = sum(len(c) for c in acols)
    Ah = dcsc_from_cols(m, len(acols), acols, np.array(av)[rng.integers(0, len(av), na)])
    U0, T0, S0, ST0 = 0, NUNIT, 2 * NUNIT, 2 * NUNIT + NSEVEN
    bcols, table = [], []
    for f, z in (boundary_pairs() if pairs is None else pairs):
        assert 1 <= z <= f <= 2 * z and z <= NUNIT
        q = z // 7 if mixed else 0                  # 7-row columns 0..q-1 cover P[0, 7q)
        q2 = min(q, (f - z) // 7)                   # their twins
        rem = f - z - 7 * q2                        # twin units 7 q2 .. 7 q2 + rem - 1 (rows inside P[0, z))
        assert 7 * q2 + rem <= z
        ks = np.concatenate([U0 + np.arange(7 * q, z), T0 + 7 * q2 + np.arange(rem), S0 + np.arange(q),
                             ST0 + np.arange(q2)])
        for _ in range(3):
            bcols.append(np.sort(ks))
            table.append((f, z))
    order = rng.permutation(len(bcols))
    bcols = [bcols[i] for i in order]
    table = [table[i] for i in order]
    nb = sum(len(c) for c in bcols)
    Bh = dcsc_from_cols(len(acols), len(bcols), bcols, np.array(bv)[rng.integers(0, len(bv), nb)])
    return Ah, Bh, table


def merge_minplus_parts(m=6000, n=120, seed=4):
    """three host partials of one shape for a min-plus MergeAll, and the expected merge
    (numpy: the elementwise min over the partials that hold a position).  Positions held
    by ONE partial carry -0.0, +0.0, +inf, DBL_MAX and ordinary values (a merge must hand
    them through unchanged); shared positions carry distinct nonzero finite values, so no
    +-0 ties.  Four dense columns make the merge product's big columns."""
    rng = np.random.default_rng(seed)
    dens = np.full(n, 0.01)
    dens[[3, 40, 41, 119]] = 0.6
    held = rng.random((3, n, m)) < dens[None, :, None]           # [part, col, row]
    lone = held.sum(0) == 1
    vals = rng.permutation(3 * n * m).reshape(3, n, m) * 0.5 - 1e5 + 0.25  # distinct, finite, never zero
    special = np.array([-0.0, 0.0, INF, DBL_MAX, -DBL_MAX, 2.0 ** -1070])[rng.integers(0, 6, (n, m))]
    vals = np.where(lone[None] & (rng.random((n, m)) < 0.7)[None], special[None], vals)
    parts = []
    for p in range(3):
        cols, rows = np.nonzero(held[p])
        jc, start = np.unique(cols, return_index=True)
        parts.append(dict(m=m, n=n, cp=np.append(start, len(rows)).astype(np.int64), jc=jc.astype(np.int32),
                          ir=rows.astype(np.int32), val=vals[p][cols, rows]))
    low = np.where(held, vals, INF).min(0)    # (an absent entry never wins: +inf loses or ties with a held +inf)
    cols, rows = np.nonzero(held.any(0))
    jc, start = np.unique(cols, return_index=True)
    want = dict(m=m, n=n, cp=np.append(start, len(rows)).astype(np.int64), jc=jc.astype(np.int32),
                ir=rows.astype(np.int32), val=low[cols, rows])
    return parts, want


def panel_edge_rows(m):
    """Bd(m): the first bitmap words' edges, the last rows, and the rows around every panel edge"""
    rows = {0, 31, 32, 63, 64, m - 2, m - 1}
    for p in range(1, (m + PANEL - 1) // PANEL + 1):
        rows |= {p * PANEL - 1, p * PANEL, p * PANEL + 1}
    return np.array(sorted(r for r in rows if 0 <= r < m), np.int64)


def panel_edge_operands(m, sr="plus", nhub=12, hub_rows=3000, nedge=700, seed=9):
    """A: nhub hub columns of Bd(m) plus hub_rows rows from a 20000-row pool, and nedge
    columns holding exactly Bd(m).  B: columns of 2..6 hubs each (dense big columns) and
    one column of all the nedge boundary-only columns (a big column whose products all
    land on boundary rows).  Dyadic values by row class: exact in any order."""
    rng = np.random.default_rng(seed)
    bd = panel_edge_rows(m)
    pool = np.setdiff1d(rng.choice(m, min(20000, m), replace=False), bd)
    acols = [np.union1d(bd, rng.choice(pool, hub_rows, replace=False)) for _ in range(nhub)] + [bd] * nedge
    bcols = [np.sort(rng.choice(nhub, int(rng.integers(2, 7)), replace=False)) for _ in range(10)]
    bcols.append(nhub + np.arange(nedge))
    bcols += [np.sort(np.concatenate([rng.choice(nhub, 2, replace=False), nhub + rng.choice(nedge, 300, replace=False)]))]
    Ah = dcsc_from_cols(m, nhub + nedge, acols)
    Bh = dcsc_from_cols(nhub + nedge, len(bcols), bcols)
    pal = dict(A=[[0.0, -0.0], [0.25, -2.25, 3.0, 1024.125, -1.0], [2.0 ** -140, -3 * 2.0 ** -141], [0.0, -0.0, 1.0]],
               B=_B_PLUS) if sr == "plus" else PALETTES["minplus"]
    return with_palette(Ah, Bh, pal, rng)


# --------------------------------------------------------------------------
# unlike pieces of one phased multiply (tests/test_gpu_aprep_cache.py; the blocks are
# checked against the thresholds without a device in tests/test_aprep_cases_cpu.py)
#
# One MemEfficientSpGEMM / PANEL SUMMA call keeps A's preparation (column map, panel
# map, f32 / f64 value records, the f32-exact and integral verdicts, max |a|) for all its
# multiplies; what a piece builds and what it takes over depends on the pieces before
# it.  A is panel_group_operands()'s A (m = 2^20 + 77: 5 row panels; 4200 stored
# columns, ~328 k entries) followed by APREP_EMPTY_A empty columns, which give the thin
# columns their flops-free entries (A's shortest stored column has 8 rows, and a thin
# column needs fewer than R / 4 = 1.25 products per B entry).  B is P blocks of
# APREP_W columns, one kind each, so that the phase cuts p * (B.n / P) fall between
# the blocks and the phase plan's sample (column ids that are multiples of 256) is
# column 0 of every block.
# --------------------------------------------------------------------------
APREP_ENTRIES, APREP_RVD_FLOPS = 64, 4   # cbg.local_aprep_bounds() (tied by test_aprep_bounds_are_the_tested_ones)
LOW_CUT_FLOPS = 1024                     # csrc/cbg_local.hip LOW_CUT_FLOPS: the cut where the lower-cut rule fires
GROUP_PRODUCTS = 4096                    # csrc/cbg_local.hip: groups of g panels where flops * g / R <= 4096
THIN_RATIO = 4                           # csrc/cbg_local.hip THIN_RATIO: thin when flops * 4 < B entries * R (R >= 4)
APREP_W = 256
APREP_EMPTY_A = 6000
_AP_HEAVY, _AP_LIGHT, _AP_LOCAL = 3000, 1000, 200   # panel_group_operands' A columns: 100 rows / 8 rows / 100 rows in panel 0
APREP_HEAVY_B = float(1 << 20)           # B_heavy's one large value, on A's column 0 (which holds int_big's 2^24)
APREP_KINDS = ("small", "empty", "lean", "rich", "thin", "B_half", "B_zero", "B_heavy")
APREP_RICH_LIKE = ("rich", "B_half", "B_zero", "B_heavy")
APREP_SEQUENCES = {
    "a": ["small", "lean", "rich", "lean", "empty", "rich", "thin"],
    "b": ["rich", "lean", "small", "rich"],
    "c": ["small", "small", "B_half", "rich", "B_zero", "rich", "B_heavy", "rich"],
    # (c)'s first piece with big columns is B_half, so a B verdict wrongly kept from the
    # first such piece would be "not integral" for all of (c) and cost no bits; here the
    # first one is integral and the unlike ones follow
    "d": ["rich", "B_half", "rich", "B_zero", "B_heavy", "lean"],
}
APREP_A_VALUES = {"int": ("plus", "minplus"), "int_big": ("plus", "minplus"), "f32": ("plus",), "f64": ("plus",)}
_APREP_CACHE = {}


def aprep_A(values):
    """A with one of the four value sets: `int` nonzero integers of magnitude <= 4,
    `int_big` the same with A's first entry (column 0) = 2^24, `f32` / `f64` the palettes
    of that name (values by row class: every plus-times sum is exact)"""
    if "A" not in _APREP_CACHE:
        Ah = panel_group_operands()[0]
        Ah = dict(Ah, n=Ah["n"] + APREP_EMPTY_A)
        assert len(Ah["jc"]) == _AP_HEAVY + _AP_LIGHT + _AP_LOCAL and int(Ah["jc"][-1]) < Ah["n"] - APREP_EMPTY_A
        _APREP_CACHE["A"] = Ah
    if ("A", values) not in _APREP_CACHE:
        Ah = _APREP_CACHE["A"]
        pal = "int" if values == "int_big" else values
        dummy = dict(ir=np.zeros(0, np.int32))
        A = with_palette(Ah, dummy, pal, np.random.default_rng(23))[0]
        if values == "int_big":
            A["val"] = A["val"].copy()
            A["val"][0] = float(1 << 24)
        _APREP_CACHE[("A", values)] = A
    return _APREP_CACHE[("A", values)]


def _aprep_block(kind, rng):
    """the columns of one block: a list of (rows of B = columns of A, values), at most
    APREP_W of them; column 0 is a big column in every kind that has one.  All values are
    nonzero integers (|v| <= 2, and 1 in the columns of more than 63 entries: every
    column's sum of |values| stays below 128 = 2^31 / 2^24 outside the thin columns)
    but for the one entry that names B_half, B_zero and B_heavy."""
    H0, L0, LOC0, E0 = 0, _AP_HEAVY, _AP_HEAVY + _AP_LIGHT, _AP_HEAVY + _AP_LIGHT + _AP_LOCAL

    def col(lo, n, cnt, mag=2):
        rows = np.sort(lo + rng.choice(n, int(cnt), replace=False))
        return rows, (rng.integers(1, mag + 1, len(rows)) * rng.choice([-1, 1], len(rows))).astype(np.float64)

    def heavy(lo, hi, mag=2):
        return col(H0, _AP_HEAVY, rng.integers(lo, hi + 1), mag)

    def small(n):   # <= 1000 flops: 2..10 heavy columns, or 2..60 light ones (8 rows each)
        return [heavy(2, 10) if i % 2 else col(L0, _AP_LIGHT, rng.integers(2, 61)) for i in range(n)]

    def mid(n):     # LOW_CUT_FLOPS < flops <= BIG_FLOPS: the columns the lower cut would move
        return [heavy(12, 38) for _ in range(n)]

    if kind == "empty":
        return []
    if kind == "small":
        return small(200) + mid(20)
    if kind == "lean":    # one big column of 50 entries; the mid columns outweigh it: the 4096 cut stays
        return [heavy(50, 50)] + small(60) + mid(6)
    if kind == "thin":    # an ordinary big column, three thin ones (5500 entries on empty A columns each)
        cols = [heavy(50, 50)]
        for nh in (50, 55, 60):
            r0, v0 = col(E0, APREP_EMPTY_A, 5500)
            r1, v1 = heavy(nh, nh)
            cols.append((np.concatenate([r1, r0]), np.concatenate([v1, v0])))
        return cols + small(30)
    assert kind in APREP_RICH_LIKE, kind
    cols = [heavy(58, 58)]
    special = len(cols)                                    # the first single-panel hash column
    cols += [heavy(105, 125, mag=1) for _ in range(44)]    # > 2 x 4096 x R / 4 flops: (column, panel) pairs, hash slabs
    cols += [heavy(42, 51) for _ in range(94)]             # <= 5120 flops: panel groups of 4
    cols += [heavy(52, 60) for _ in range(71)]             # <= 10240 flops: panel groups of 2
    cols += [col(LOC0, _AP_LOCAL, rng.integers(45, 61)) for _ in range(10)]           # > 4096 products in panel 0
    cols += [col(LOC0, _AP_LOCAL, rng.integers(105, 126), mag=1) for _ in range(6)]   # ... as single pairs: bitmap slabs
    cols += mid(8) + small(20)                             # the lower cut fires: the mid columns run as big ones
    rows, vals = cols[special]
    if rows[0] != 0:
        rows[0] = 0     # A's column 0 (still ascending and distinct)
    vals[0] = {"rich": vals[0], "B_half": 0.5, "B_zero": 0.0, "B_heavy": APREP_HEAVY_B}[kind]
    return cols


def aprep_B(seq):
    """(B, kinds) of sequence `seq` (APREP_SEQUENCES): block p holds columns [p * APREP_W, (p + 1) * APREP_W)"""
    if ("B", seq) not in _APREP_CACHE:
        kinds = APREP_SEQUENCES[seq]
        rng = np.random.default_rng(100 + sorted(APREP_SEQUENCES).index(seq))
        cols, vals = [], []
        for kind in kinds:
            blk = _aprep_block(kind, rng)
            assert len(blk) <= APREP_W
            cols += [c for c, _ in blk] + [np.zeros(0, np.int64)] * (APREP_W - len(blk))
            vals += [v for _, v in blk]
        k = _AP_HEAVY + _AP_LIGHT + _AP_LOCAL + APREP_EMPTY_A
        Bh = dcsc_from_cols(k, len(cols), cols, np.concatenate(vals))
        _APREP_CACHE[("B", seq)] = (Bh, list(kinds))
    return _APREP_CACHE[("B", seq)]


def aprep_pieces(Bh, P):
    """the P column pieces of MemEfficientSpGEMM: cuts at p * (B.n // P), the last to B.n"""
    w = Bh["n"] // P
    out, rest = [], Bh
    for p in range(P - 1):
        left, rest = split_cols_host(rest, w)
        out.append(left)
    return out + [rest]


def aprep_refs(seq, values, sr):
    """the oracle's C of every piece of sequence `seq` (computed once, shared, left unchanged)"""
    key = ("C", seq, values, sr)
    if key not in _APREP_CACHE:
        Bh, kinds = aprep_B(seq)
        A = aprep_A(values)
        _APREP_CACHE[key] = [oracle_local(A, Bp, sr) for Bp in aprep_pieces(Bh, len(kinds))]
    return _APREP_CACHE[key]


def aprep_piece_facts(Ah, Bp):
    """what the multiply's host rules make of one piece, from the oracle's flops per column
    and the documented thresholds: the big-column cut (BIG_FLOPS, or LOW_CUT_FLOPS where
    columns in between exist and the columns above BIG_FLOPS carry at least half of the
    piece's flops; m <= 2^22 holds), the big and thin columns under that cut, their B
    entries and flops, and B's integrality, largest |value| and largest column sum of |values|"""
    nz = len(Bp["jc"])
    if nz == 0:
        none = np.zeros(0, np.int64)
        return dict(stored=0, cut=0, nbig=0, nthin=0, big_entries=0, big_flops=0, over_flops=0, flops=0, low_cond=False,
                    moved=0, col_flops=none, col_big=none.astype(bool), col_thin=none.astype(bool), b_integral=True,
                    b_max=0.0, b_colsum=0.0, b_zeros=0)
    f = oracle_symbolic(Ah, Bp)[0].astype(np.int64)
    ne = np.diff(Bp["cp"]).astype(np.int64)
    assert (ne >= 2).all()     # (a single-entry column is a scaled copy of A's column whatever its flops)
    R = (Ah["m"] + PANEL - 1) // PANEL
    thin_R = R if R >= 4 else 0

    def classes(cut):
        over = f > cut
        thin = over & (f * THIN_RATIO < ne * thin_R)
        return over & ~thin, thin

    big, thin = classes(BIG_FLOPS)
    moved = (f > LOW_CUT_FLOPS) & (f <= BIG_FLOPS)
    low_cond = bool(2 * int(f[big | thin].sum()) >= int(f.sum()))
    cut = LOW_CUT_FLOPS if (moved.any() and low_cond and Ah["m"] <= (1 << 22)) else BIG_FLOPS
    big, thin = classes(cut)
    v = np.asarray(Bp["val"], np.float64)
    colsum = np.add.reduceat(np.abs(v), Bp["cp"][:-1].astype(np.int64))
    return dict(stored=nz, cut=cut, nbig=int(big.sum()), nthin=int(thin.sum()), big_entries=int(ne[big].sum()),
                big_flops=int(f[big].sum()), over_flops=int(f[f > BIG_FLOPS].sum()), flops=int(f.sum()),
                low_cond=low_cond, moved=int(moved.sum()), col_flops=f, col_big=big, col_thin=thin,
                b_integral=bool((v == np.trunc(v)).all() and (v != 0).all() and (np.abs(v) <= 2.0 ** 24).all()),
                b_max=float(np.abs(v).max()), b_colsum=float(colsum.max()), b_zeros=int((v == 0).sum()))


# --------------------------------------------------------------------------
# tall tiles (tests/test_gpu_tall_tiles.py; the routes are checked without a device in
# tests/test_tall_tiles_cpu.py): operands whose B columns are built for one route each
# at a given m, and the routes the documented rules give them
#
# The local multiply switches by the number of row panels R = ceil(m / 2^18) as well as by
# flops and nonzeros.  tall_operands() gives every B column its own A columns, so a
# column's flops, its products per row range and its nonzeros per row range are what
# the spec says, whatever m is; nothing here allocates O(m).
# --------------------------------------------------------------------------
TALL_HASH_T = (512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192)   # csrc/cbg_local.hip CBG_HASH_TABLES
TALL_RANK_MIN = 683            # RANK_SLABS_MIN, GRANK_SLABS_MIN: sparse slabs of more nonzeros are ranked
TALL_GRANK_SPAN = 1 << 22      # GRANK_SPAN_LOG: rows a group rank slab may span
TALL_GRANK_PMAX = 4096         # GRANK_PMAX: a group's slab of more products is a hash slab (SLAB_MANYP)
TALL_SPARSE_MAX = 4096         # SPARSE_SLAB_MAX (products of a hash-mode pair), SPARSE_NNZ_MAX (nonzeros of a hash slab)
TALL_GROUP_TABLE = 8192        # GROUP_T: the group symbolic's table; it takes a group of products * 3 / 2 <= this
TALL_BIG_BS = 512              # BIG_BS: B entries a group unit stages at once
TALL_ESC_FLOPS = 512           # kSymThr[SYM_FUSED_LAST]: columns of fewer flops run expand-sort-compress
TALL_SLAB_KEYS = 8192          # SLAB_KEYS_MAX, with 16 slab classes: (class, panel) keys while 16 R <= 8192
TALL_BITMAP_SMALL = 3056       # SLAB_SMALL_CAP: bitmap slabs of no more nonzeros are `small` under either accumulation


def panel_rows(m, r0, r1=None):
    """[lo, hi): the rows of panels r0..r1 of a tile of m rows"""
    r1 = r0 if r1 is None else r1
    return r0 * PANEL, min((r1 + 1) * PANEL, m)


def _distinct_rows(rng, lo, hi, n, must):
    """n distinct rows of [lo, hi) in random order, `must` among them; no array of hi - lo entries
    unless that is small"""
    must = np.unique(np.asarray(must, np.int64))
    assert len(must) <= n <= hi - lo and (len(must) == 0 or (lo <= must[0] and must[-1] < hi)), (lo, hi, n, must)
    if hi - lo <= PANEL:
        rest = np.setdiff1d(np.arange(lo, hi, dtype=np.int64), must)
        rest = rng.choice(rest, n - len(must), replace=False)
    else:
        rest = np.zeros(0, np.int64)
        while len(rest) < n - len(must):
            draw = rng.integers(lo, hi, 2 * (n - len(must)) + 16)
            rest = np.setdiff1d(np.union1d(rest, draw), must)
        rest = rng.permutation(rest)[:n - len(must)]
    return rng.permutation(np.concatenate([must, rest]))


def tall_operands(m, spec, values="int", seed=0):
    """(Ah, Bh, plan).  spec: one dict per B column, in column order:
        route    the route the column is meant for (tall_plan's names: "copy", "esc", "small",
                 "thin", "g64" ... "g2", "g1"); compared with the prediction in plan["routes"]
        nb       its B entries; each is an A column of its own
        regions  [(lo, hi, products, nnz, must), ...]: disjoint row ranges; the column has
                 exactly `products` products in [lo, hi), on exactly min(products, nnz)
                 distinct rows, the rows `must` among them (needs products >= nnz >= len(must)
                 for every one of them to appear).  The products are dealt to the nb A columns
                 in turn, each taking the next rows of the range's (shuffled) row pool
                 cyclically: sums form wherever products > nnz.
    The column's flops are the sum of its products.  values: `int` integers 1..4 in A and
    1..2 in B (exact in any order; IACC), `half` the same with A + 0.5 (f32-exact, not
    integral: the f64 slabs), `random` U(-1, 1) in both.  plan = tall_plan(Ah, Bh) with
    plan["intended"] the spec's routes."""
    rng = np.random.default_rng(seed)
    acols, bcols = [], []
    for c in spec:
        nb = int(c["nb"])
        rows, owner = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        last_hi = 0
        for lo, hi, products, nnz, must in sorted(c["regions"], key=lambda g: g[0]):
            assert last_hi <= lo < hi <= m and len(must) <= nnz <= hi - lo, (lo, hi, nnz, last_hi, m)
            last_hi = hi
            base, rem = divmod(int(products), nb)
            assert base + (1 if rem else 0) <= nnz, (c["route"], products, nb, nnz)
            pool = _distinct_rows(rng, lo, hi, nnz, must)
            rows.append(pool[np.arange(products) % nnz])           # one sweep over the pool, dealt in turn
            owner.append(np.repeat(np.arange(nb), base + (np.arange(nb) < rem)))
        rows, owner = np.concatenate(rows), np.concatenate(owner)
        o = np.lexsort((rows, owner))
        cut = np.searchsorted(owner[o], np.arange(nb + 1))
        bcols.append(np.arange(len(acols), len(acols) + nb))
        acols += [rows[o][cut[j]:cut[j + 1]] for j in range(nb)]
    Ah = dcsc_from_cols(m, len(acols), acols)
    Bh = dcsc_from_cols(len(acols), len(bcols), bcols)
    Ah, Bh = tall_values(Ah, Bh, values, seed)
    plan = tall_plan(Ah, Bh)
    plan["intended"] = [c["route"] for c in spec]
    return Ah, Bh, plan


def tall_values(Ah, Bh, values, seed=0):
    """copies of Ah, Bh with the same structure and the values of tall_operands' `values`"""
    rng = np.random.default_rng([seed, 77])
    na, nbs = len(Ah["ir"]), len(Bh["ir"])
    if values == "random":
        av, bv = rng.uniform(-1.0, 1.0, na), rng.uniform(-1.0, 1.0, nbs)
    else:
        assert values in ("int", "half"), values
        av = rng.integers(1, 5, na).astype(np.float64) + (0.5 if values == "half" else 0.0)
        bv = rng.integers(1, 3, nbs).astype(np.float64)
    return dict(Ah, val=av), dict(Bh, val=bv)


def tall_sparse_class(nnz, span, products=0, group=False):
    """csrc/cbg_local.hip slab_class for a sparse (hash-mode) slab: a rank slab above
    TALL_RANK_MIN nonzeros where it spans one panel; a group rank slab above it where it is a
    group's slab of <= TALL_GRANK_PMAX products spanning <= 2^22 rows; else the smallest hash
    table of load <= 2/3"""
    if nnz > TALL_RANK_MIN and span <= PANEL:
        return "rank_N%d" % (1024 if nnz <= 1024 else 2048 if nnz <= 2048 else 4096)
    if nnz > TALL_RANK_MIN and group and products <= TALL_GRANK_PMAX and PANEL < span <= TALL_GRANK_SPAN:
        return "group_rank_N%d" % (2048 if nnz <= 2048 else 4096)
    return "hash_T%d" % next((t for t in TALL_HASH_T if 2 * t >= 3 * nnz), TALL_HASH_T[-1])


def thin_key_bits(m, nthin):
    """csrc/cbg_thin.hip thin_any: bits of a (column, row) key; 32-bit keys while they are <= 32"""
    rowbits = colbits = 1
    while (1 << rowbits) < m:
        rowbits += 1
    while (1 << colbits) < nthin:
        colbits += 1
    return rowbits + colbits


def tall_plan(Ah, Bh):
    """The routes the documented rules of csrc/cbg_local.hip / cbg_thin.hip give every stored B
    column of A * B, for m > 2^22 rows (the big cut is then 4096 flops), from the oracle's flops
    per column and the operands themselves; no device.

    Column routes (k_classify; plan_symbolic_bins): one B entry: "copy"; flops <= 512: "esc";
    <= 4096: "small"; above, with R >= 4 and flops * 4 < entries * R: "thin"; else the first
    group size g = 64, 32 ... 2 with g <= R and flops <= 4096 * R // g: "g<g>"; else "g1".

    Units (sym_big_columns, k_sym_panel, sym_group, sym_pair): a column of class g has
    ceil(R / g) units of panels [r0, min(r0 + g, R) - 1], counted in sym_group_units (g > 1)
    or sym_panel_units (g = 1) whether or not any product falls into them.  A group unit is
    handed to k_sym_deferred (sym_deferred_units), which runs its panels one by one, when it
    is a single panel (the ragged last group: r1 == r0, empty or not), when the column has
    more than 512 B entries, when its products * 3 / 2 exceed the 8192-slot table (products >
    5461) or when its nonzeros exceed 4096; else, if it has any nonzero, it is ONE sparse slab
    over the group's rows, filed under its first panel.  A single panel (class g1 or deferred)
    with <= 512 B entries and <= 4096 products is one sparse slab over the panel's rows; with
    more it is a bitmap pair (here: of <= 3056 nonzeros, one `bitmap_small` slab).  A sparse
    slab's launch class: tall_sparse_class."""
    m = int(Ah["m"])
    assert m > TALL_GRANK_SPAN, "the lower big-column cut (m <= 2^22) is not restated here"
    R = (m + PANEL - 1) // PANEL
    f = np.asarray(oracle_symbolic(Ah, Bh)[0], np.int64)
    ne = np.diff(Bh["cp"]).astype(np.int64)
    classes = [g for g in (64, 32, 16, 8, 4, 2) if g <= R]
    acp = np.asarray(Ah["cp"], np.int64)
    aslot = np.full(Ah["n"], -1, np.int64)
    aslot[Ah["jc"]] = np.arange(len(Ah["jc"]))
    routes, groups = [], {}
    slabs, keys = {}, []
    units = dict(sym_group_units=0, sym_panel_units=0, sym_deferred_units=0)

    def add_slab(cls, panel):
        slabs[cls] = slabs.get(cls, 0) + 1
        keys.append((cls, panel))

    def single_panel(rows, r, nb):
        pr = rows[(rows >> 18) == r]
        if len(pr) == 0:
            return
        z = len(np.unique(pr))
        lo, hi = panel_rows(m, r)
        if nb <= TALL_BIG_BS and len(pr) <= TALL_SPARSE_MAX:
            add_slab(tall_sparse_class(z, hi - lo), r)
        else:
            assert z <= TALL_BITMAP_SMALL, "bitmap pairs of more than one small slab are not restated here"
            add_slab("bitmap_small", r)

    for j in range(len(ne)):
        F, nb = int(f[j]), int(ne[j])
        if nb == 1:
            routes.append("copy")
        elif F <= TALL_ESC_FLOPS:
            routes.append("esc")
        elif F <= BIG_FLOPS:
            routes.append("small")
        elif R >= 4 and F * THIN_RATIO < nb * R:
            routes.append("thin")
        else:
            g = next((g for g in classes if F <= GROUP_PRODUCTS * R // g), 1)
            routes.append("g%d" % g)
            ks = aslot[Bh["ir"][Bh["cp"][j]:Bh["cp"][j + 1]]]
            ks = ks[ks >= 0]
            rows = np.concatenate([Ah["ir"][acp[k]:acp[k + 1]] for k in ks]).astype(np.int64)
            assert len(rows) == F
            ng = (R + g - 1) // g
            units["sym_group_units" if g > 1 else "sym_panel_units"] += ng
            glist = []
            for q in range(ng):
                r0, r1 = q * g, min(q * g + g, R) - 1
                lo, hi = panel_rows(m, r0, r1)
                gr = rows[(rows >= lo) & (rows < hi)]
                P, Z = len(gr), len(np.unique(gr))
                if g == 1:
                    single_panel(gr, r0, nb)
                    out = "panel"
                elif r1 == r0 or nb > TALL_BIG_BS or 3 * P > 2 * TALL_GROUP_TABLE or Z > TALL_SPARSE_MAX:
                    units["sym_deferred_units"] += 1
                    for r in range(r0, r1 + 1):
                        single_panel(gr, r, nb)
                    out = "deferred"
                elif Z > 0:
                    out = tall_sparse_class(Z, hi - lo, P, group=True)
                    add_slab(out, r0)
                else:
                    out = "empty"
                glist.append((r0, r1, P, Z, out))
            groups[j] = glist
    routes = np.array(routes)
    nthin = int((routes == "thin").sum())
    big = np.array([r[0] == "g" for r in routes])
    return dict(R=R, routes=list(routes), flops=f, entries=ne, groups=groups, slabs=slabs, slab_keys=keys,
                n_slabs=len(keys), n_big=int(big.sum()), thin_columns=nthin, esc_columns=int((routes == "esc").sum()),
                small_columns=int((routes == "small").sum()), copy_columns=int((routes == "copy").sum()),
                class_columns={g: int((routes == "g%d" % g).sum()) for g in classes + [1]},
                thin_key_bits=thin_key_bits(m, nthin) if nthin else 0,
                slab_keys_by_panel=16 * R <= TALL_SLAB_KEYS, **units)


def _ends(lo, hi, *more):
    return [lo, hi - 1] + [r for r in more if lo <= r < hi]


def _group_regions(m, g, cells, full_panels, tail=None):
    """regions of a column taken in groups of g panels: cells = {group: (products, nnz)} over the
    first `full_panels` panels, each group's first and last row among its rows; `tail`
    (products, nnz): the rows from panel `full_panels` on (the ragged last panel), if the tile has any"""
    out = []
    for q, (P, Z) in sorted(cells.items()):
        lo, hi = panel_rows(m, q * g, q * g + g - 1)
        assert hi == (q + 1) * g * PANEL <= full_panels * PANEL
        out.append((lo, hi, P, Z, _ends(lo, hi)))
    if tail and m > full_panels * PANEL:
        lo = full_panels * PANEL
        out.append((lo, m, tail[0], min(tail[1], m - lo), _ends(lo, m)))
    return out


def tall_spec_65(m=(1 << 24) + 77):
    """R = 65: the 64-panel class holds the columns of 4097..4160 flops (4096 * 65 // 64), as
    panels 0..63 and the lone ragged panel 64 (77 rows), which is always a deferred unit"""
    assert (m + PANEL - 1) // PANEL == 65
    G, H2 = 1 << 24, 1 << 23
    anywhere = lambda P, Z: [(0, m, P, Z, _ends(0, m))]
    return [
        # the class's upper edge: 4110 products (> 4096: SLAB_MANYP) on 1500 rows of the group, 50 in panel 64
        dict(route="g64", nb=50, regions=[(0, G, 4110, 1500, _ends(0, G)), (G, m, 50, 40, _ends(G, m))]),
        # its lower edge; nothing in panel 64 (an empty deferred unit); 700 nonzeros over 2^24 rows stay a hash slab
        dict(route="g64", nb=40, regions=[(0, G, 4097, 700, _ends(0, G))]),
        # only rows of panel 64: an empty group, and 4130 products on 77 rows in the deferred panel (a bitmap pair)
        dict(route="g64", nb=60, regions=[(G, m, 4130, 77, _ends(G, m))]),
        # the control: 32-panel groups (4161..8320 flops), at its lower edge and inside
        dict(route="g32", nb=40, regions=[(0, H2, 2100, 500, _ends(0, H2)), (H2, G, 2061, 684, _ends(H2, G))]),
        dict(route="g32", nb=100, regions=[(0, H2, 3900, 1200, _ends(0, H2)), (H2, G, 3900, 700, _ends(H2, G)),
                                           (G, m, 200, 60, _ends(G, m))]),
        dict(route="thin", nb=400, regions=anywhere(4200, 1500)),
        dict(route="small", nb=20, regions=anywhere(3000, 2000)),
        dict(route="esc", nb=3, regions=anywhere(300, 200)),
        dict(route="copy", nb=1, regions=anywhere(500, 500)),
    ]


def tall_spec_512(m):
    """m = 2^27 (R = 512: the slab list keyed by class and panel) or 2^27 + 5 (R = 513: by class
    alone; the last group of every class is the 5-row panel 512, a deferred unit): one column
    per group class 64 .. 4 with its flops in the upper half of the class's range, every full
    group populated with <= 4096 products, its first and last row included; a second 16-panel
    column with the groups that leave the group path"""
    R = (m + PANEL - 1) // PANEL
    assert R in (512, 513) and m >= (1 << 27)
    tail = (10, 5)
    z16 = (683, 684, 2048, 2049)     # the group rank classes' edges: hash_T1536 | N2048 | N2048 | N4096
    odd = {q: (3750, 1200) for q in range(21)}
    odd.update({21: (4500, 2500),    # > 4096 products: no group rank slab (a hash slab)
                22: (6000, 3000),    # > 5461 products: deferred, 16 single panels
                23: (5461, 4096),    # the largest group the table takes, the most nonzeros of a hash slab
                24: (5462, 1000),    # one product more: deferred
                25: (5000, 4097)})   # one nonzero more: deferred
    anywhere = lambda P, Z: [(0, m, P, Z, _ends(0, m))]
    return [
        dict(route="g64", nb=64, regions=_group_regions(m, 64, {q: (3750, 800) for q in range(8)}, 512, tail)),
        dict(route="g32", nb=100, regions=_group_regions(m, 32, {q: (3750, 1000) for q in range(16)}, 512, tail)),
        dict(route="g16", nb=128, regions=_group_regions(m, 16, {q: (3750, z16[q % 4]) for q in range(32)}, 512, tail)),
        dict(route="g16", nb=128, regions=_group_regions(m, 16, odd, 512, tail)),
        dict(route="g8", nb=200, regions=_group_regions(m, 8, {q: (3900, 1500) for q in range(64)}, 512, tail)),
        dict(route="g4", nb=256, regions=_group_regions(m, 4, {q: (3900, 2500) for q in range(128)}, 512, tail)),
        dict(route="esc", nb=4, regions=anywhere(400, 300)),
        dict(route="esc", nb=2, regions=anywhere(512, 256)),
        dict(route="esc", nb=3, regions=anywhere(40, 30)),
        dict(route="small", nb=20, regions=anywhere(3000, 2000)),
        dict(route="small", nb=2, regions=anywhere(513, 300)),
        dict(route="small", nb=8, regions=anywhere(4096, 1000)),
        dict(route="copy", nb=1, regions=anywhere(100, 100)),
    ]


TALL_MAX_M = (1 << 31) - 2     # the tallest tile the ABI admits (m < INT32_MAX)


def tall_spec_8192(m=TALL_MAX_M):
    """m = 2^31 - 2 (R = 8192, row ids up to 2^31 - 3): three 64-panel-class big columns
    (flops <= 524288; not thin: flops >= 2048 x entries), three thin columns (64-bit keys: 31 row
    bits), ESC, block-hash and single-entry columns; rows 0, 2^31 - 2^18 - 1, m - 2 and m - 1"""
    R = (m + PANEL - 1) // PANEL
    assert R == 8192
    last = (R - 1) * PANEL          # first row of the last panel (2^18 - 2 rows)
    edge = [0, last - 1, m - 2, m - 1]

    def groups(qs, P, Z):
        out = []
        for q in qs:
            lo, hi = panel_rows(m, 64 * q, 64 * q + 63)
            out.append((lo, hi, P, Z, _ends(lo, hi, *edge)))
        return out

    anywhere = lambda P, Z: [(0, m, P, Z, edge)]
    qa = [0, 1, 2, 3] + list(range(8, 128, 6)) + [126, 127]
    qb = list(range(5, 125, 6))
    return [
        dict(route="g64", nb=40, regions=groups(qa, 3840, 1000)),
        # the last group's products all in the last panel, > 5461 of them: deferred, and there a bitmap pair
        # whose last fine range ends past 2^31
        dict(route="g64", nb=40, regions=groups(qb, 3840, 684) + [(last, m, 6000, 2000, [last, m - 2, m - 1])]),
        dict(route="g64", nb=48, regions=groups(qa[1:] + [4], 3840, 3000)),
        dict(route="thin", nb=8, regions=anywhere(5000, 3000)),
        dict(route="thin", nb=9, regions=anywhere(4097, 1000)),
        dict(route="thin", nb=300, regions=anywhere(6000, 1500)),
        dict(route="esc", nb=3, regions=anywhere(300, 200)),
        dict(route="esc", nb=2, regions=anywhere(512, 256)),
        dict(route="esc", nb=5, regions=anywhere(9, 4)),
        dict(route="small", nb=10, regions=anywhere(2000, 1500)),
        dict(route="copy", nb=1, regions=anywhere(300, 300)),
        dict(route="copy", nb=1, regions=anywhere(5000, 5000)),     # more flops than the big cut: the chunked copy
    ]


_TALL_CACHE = {}


def tall_case(name):
    """(Ah, Bh, plan) of a named case with the `int` values, built once: r65, r512, r513, r8192"""
    if name not in _TALL_CACHE:
        m, spec = {"r65": ((1 << 24) + 77, tall_spec_65), "r512": (1 << 27, tall_spec_512),
                   "r513": ((1 << 27) + 5, tall_spec_512), "r8192": (TALL_MAX_M, tall_spec_8192)}[name]
        _TALL_CACHE[name] = tall_operands(m, spec(m), "int", seed=sorted(("r65", "r512", "r513", "r8192")).index(name))
    return _TALL_CACHE[name]


def tall_reference(name, values, sr):
    """(A, B, oracle's C) of a named case under `values`, computed once, shared, left unchanged"""
    key = (name, values, sr)
    if key not in _TALL_CACHE:
        Ah, Bh, _ = tall_case(name)
        A, B = (Ah, Bh) if values == "int" else tall_values(Ah, Bh, values)
        _TALL_CACHE[key] = (A, B, oracle_local(A, B, sr))
    return _TALL_CACHE[key]


def thin_key_operands(m, nthin, arows):
    """nthin thin columns and nothing else, for the thin pass's key width (32-bit keys while
    rowbits(m) + colbits(nthin) <= 32).  Unlike tall_operands the B columns SHARE A's columns:
    the inline path (A's columns of one or two rows held in the column map's records) is taken
    where nnz(A) <= 2 x A's stored columns and the flops are >= 4 nnz(A), so every A entry has
    to be used several times.  arows = 2: A has 3000 columns of one and two rows alternately
    and every B column 2900 of them (>= 4300 flops); arows = 8: 700 columns of 8 rows, 600 per B
    column (4800 flops).  Rows come from a pool of 1500 (0, 2^27 - 1 and m - 1 among them): the
    products of a column collide.  Integer values (exact in any order)."""
    rng = np.random.default_rng([m % 1000, nthin, arows])
    K, nb = (3000, 2900) if arows == 2 else (700, 600)
    must = np.unique([0, (1 << 27) - 1, m - 1])
    pool = _distinct_rows(rng, 0, m, 1500, must)
    rest = np.setdiff1d(pool, must)
    lens = (1 + np.arange(K) % 2) if arows == 2 else np.full(K, arows)
    acols = [np.sort(rng.choice(pool, L, replace=False)) for L in lens]
    special = 1 + 2 * np.arange(len(must))    # columns 1, 3, 5 (two rows where arows = 2) hold the edge rows
    for k, r in zip(special, must):
        acols[k] = np.sort(np.append(rng.choice(rest, lens[k] - 1, replace=False), r))
    others = np.setdiff1d(np.arange(K), special)
    bcols = [np.sort(np.append(rng.choice(others, nb - len(special), replace=False), special)) for _ in range(nthin)]
    Ah = dcsc_from_cols(m, K, acols, rng.integers(1, 5, int(lens.sum())).astype(np.float64))
    Bh = dcsc_from_cols(K, nthin, bcols, rng.integers(1, 3, nthin * nb).astype(np.float64))
    return Ah, Bh
