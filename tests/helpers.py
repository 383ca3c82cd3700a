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
