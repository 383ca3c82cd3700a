"""Order-exact NumPy restatement of y = A x on PlusTimesSRing<double,double> and
MinPlusSRing<double,double> (csrc/cbg_spmv.hip, include/cbg.h): this file is the statement of the
sum order; the GPU tests compare the device with it by bits on inexact values.

The products of row i are mul(a(i, j), x[j]) over the stored (i, j) whose j takes part, in ascending
j, each rounded on its own.  With a dense x every stored column takes part (a stored entry times
x[j] = 0 is still a product); with a sparse x exactly the columns of xind.

The order of a row's sum depends on the number L of its products alone:

  L <= 16     G = 16 lanes
  L <= 4096   G = 64 lanes
  longer      chunks of 4096 products (the last one shorter), each reduced as a 64-lane row; the
              chunk results are folded one after another in chunk order

Lane l starts at the device's identity (-0.0 for PlusTimes, +inf for MinPlus) and folds products
l, l + G, l + 2G, ... one after another; the lanes are combined by the xor tree over distances 1, 2,
4, ... (colsum_ref.lane_sum with lanes=G; it starts its lanes at +0.0, which differs from -0.0 only
for a row whose products are all -0.0: that row sums to -0.0 here).  add of MinPlus is
b < a ? b : a, its mul is inf_plus: DBL_MAX if either side is DBL_MAX, else a + b.

  dense result   y[i] = add(id, r_i) with the reference's id, 0.0 and DBL_MAX; id for a row without
                 a stored entry.  (So an all -0.0 row gives +0.0 here and -0.0 in the sparse result.)
  sparse result  one entry per row with a product, rows ascending, value r_i itself.

On a grid the columns are cut at `cuts` (ascending column ids: cuts = [c] gives the column blocks
[0, c) and [c, n)); each block's products are reduced by the rules above (the class from the block's
count) and the blocks' results are combined with add in block order: a block without a product of
the row contributes nothing (sparse) or id (dense).  The row cuts of a grid do not matter.

A NaN in the inputs is outside the contract (an inf - inf inside a sum gives the NaN either way);
so is a MinPlus minimum that is a zero occurring with both signs.

A matrix is a DCSC dict (m, n, cp, jc, ir, val), as in colsum_ref."""
import numpy as np

from colsum_ref import DBL_MAX, cols_of, lane_sum

PLUS_TIMES, MIN_PLUS = 0, 1
GROUP_MAX, WAVE_MAX = 16, 4096  # cbg_spmv_bounds()[0:2]; WAVE_MAX is also the chunk
ID = {PLUS_TIMES: 0.0, MIN_PLUS: DBL_MAX}  # the reference's SR::id()


def mul(sr, a, x):
    a, x = np.asarray(a, np.float64), np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if sr == PLUS_TIMES:
            return a * x
        return np.where((a == DBL_MAX) | (x == DBL_MAX), DBL_MAX, a + x)


def add(sr, a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        if sr == PLUS_TIMES:
            return float(np.float64(a) + np.float64(b))
    return float(b) if b < a else float(a)


def _lanes_min(p, g):
    rounds = -(-len(p) // g)
    pad = np.full(rounds * g, np.inf)
    pad[:len(p)] = p
    acc = np.full(g, np.inf)
    for row in pad.reshape(rounds, g):
        acc = np.where(row < acc, row, acc)
    lane, d = np.arange(g), 1
    while d < g:
        other = acc[lane ^ d]
        acc = np.where(other < acc, other, acc)
        d *= 2
    return float(acc[0])


def lanes_reduce(p, sr, g):
    """g lanes over the products p (at least one)"""
    if sr == MIN_PLUS:
        return _lanes_min(p, g)
    r = lane_sum(p, lanes=g)
    if r == 0.0 and np.all((p == 0.0) & np.signbit(p)):
        return -0.0  # the lanes start at -0.0
    return r


def row_reduce(p, sr, lanes=None):
    """r of a row (or of one column block's part of it) with the products p, len(p) >= 1.
    lanes: another lane count than the device's for the rows of at most 4096 products"""
    p = np.asarray(p, np.float64)
    if len(p) <= WAVE_MAX:
        return lanes_reduce(p, sr, (GROUP_MAX if len(p) <= GROUP_MAX else 64) if lanes is None else lanes)
    acc = None
    for c in range(0, len(p), WAVE_MAX):
        r = lanes_reduce(p[c:c + WAVE_MAX], sr, 64)
        acc = r if acc is None else add(sr, acc, r)
    return acc


def fold_id(sr, r):
    """add(id, r): what the dense result stores"""
    return add(sr, ID[sr], r)


_rows_cache = {}


def rows_of(t):
    """per row: (column ids ascending, values).  Cached by the identity of t's arrays"""
    key = (id(t["ir"]), id(t["val"]), t["m"])
    if key not in _rows_cache:
        col, row = cols_of(t), np.asarray(t["ir"], np.int64)
        order = np.lexsort((col, row))
        col, row, val = col[order], row[order], np.asarray(t["val"], np.float64)[order]
        at = np.searchsorted(row, np.arange(t["m"] + 1))
        _rows_cache[key] = (t["ir"], t["val"], [(col[a:b], val[a:b]) for a, b in zip(at[:-1], at[1:])])
    return _rows_cache[key][2]


def _blocks(cols, cuts):
    at = [0] + [int(np.searchsorted(cols, c)) for c in (cuts or [])] + [len(cols)]
    return [slice(a, b) for a, b in zip(at[:-1], at[1:])]


def row_lengths(t):
    return np.bincount(np.asarray(t["ir"], np.int64), minlength=t["m"])


def spmv(t, x, sr=PLUS_TIMES, cuts=None, lanes=None):
    """the dense product: m doubles"""
    x = np.asarray(x, np.float64)
    y = np.full(t["m"], ID[sr])
    for i, (cols, vals) in enumerate(rows_of(t)):
        if len(cols) == 0:
            continue
        p = mul(sr, vals, x[cols])
        acc = None
        for s in _blocks(cols, cuts):
            part = fold_id(sr, row_reduce(p[s], sr, lanes)) if s.stop > s.start else ID[sr]
            acc = part if acc is None else add(sr, acc, part)
        y[i] = acc
    return y


def spmspv(t, xind, xval, sr=PLUS_TIMES, cuts=None, lanes=None):
    """the sparse product: (row ids ascending, values)"""
    xind = np.asarray(xind, np.int64)
    inx = np.zeros(max(t["n"], 1), bool)
    inx[xind] = True
    xd = np.zeros(max(t["n"], 1))
    xd[xind] = np.asarray(xval, np.float64)
    yi, yv = [], []
    for i, (cols, vals) in enumerate(rows_of(t)):
        use = inx[cols]
        if not use.any():
            continue
        cols, vals = cols[use], vals[use]
        p = mul(sr, vals, xd[cols])
        acc = None
        for s in _blocks(cols, cuts):
            if s.stop > s.start:
                part = row_reduce(p[s], sr, lanes)
                acc = part if acc is None else add(sr, acc, part)
        yi.append(i)
        yv.append(acc)
    return np.array(yi, np.int64), np.array(yv, np.float64)


def bound(t, x, pc=1):
    """2 (L + pc) 2^-53 sum_j |a(i, j) x[j]| per row: two orderings of the same rounded products
    (each ordering's error is at most (L - 1 + pc) u sum |p| to first order; the factor 2 and the + 1
    cover the higher-order terms for every L < 2^26)"""
    x = np.asarray(x, np.float64)
    b = np.zeros(t["m"])
    for i, (cols, vals) in enumerate(rows_of(t)):
        if len(cols):
            b[i] = 2.0 * (len(cols) + pc) * 2.0 ** -53 * np.abs(vals * x[cols]).sum()
    return b


def restrict_cols(t, ids):
    """the columns `ids` of t alone (same shape): the entries that take part under a sparse x"""
    col = cols_of(t)
    keep = np.isin(col, np.asarray(ids, np.int64))
    jc, start = np.unique(col[keep], return_index=True)
    return dict(m=t["m"], n=t["n"], cp=np.append(start, int(keep.sum())).astype(np.int64), jc=jc.astype(np.int32),
                ir=np.asarray(t["ir"])[keep], val=np.asarray(t["val"], np.float64)[keep])


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)
