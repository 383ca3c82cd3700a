"""NumPy restatement of sparse indexing B(i, j) = A(ri[i], ci[j]) (SpParMat::SubsRef_SR,
SpParMat.cpp:2026-2247; SpDCCols::operator(), SpDCCols.cpp:1355-1383), of the library's
RandPerm, of SpParMat::LoadImbalance and of HipMCL's two preparation steps
(RemoveIsolated, RandPermute: MCL.cpp:476-521), with the test matrices of their tests.

A matrix is a DCSC dict (m, n, cp, jc, ir, val) of the WHOLE matrix.  Nothing is
computed with the values: they are carried by fancy indexing, so they keep their bits."""
import numpy as np

import hipmcl_ref as hr
from helpers import _mix64

GOLDEN_CASES = ("symperm", "twoperm", "increasing", "rect")


def _join(old, idx):
    """every entry with old index old[e] against the requests idx: (entry, position in idx) pairs,
    through the inverse lists of idx (a stable counting sort of it)"""
    order = np.argsort(idx, kind="stable")
    sidx = idx[order]
    lo, hi = np.searchsorted(sidx, old, "left"), np.searchsorted(sidx, old, "right")
    cnt = hi - lo
    ent = np.repeat(np.arange(len(old)), cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return ent, order[np.repeat(lo, cnt) + within]


def spref(t, ri=None, ci=None):
    """the nri x nci matrix t(ri, ci); None: all, in order"""
    row, col, val = t["ir"].astype(np.int64), hr.cols_of(t), t["val"]
    m, n = t["m"], t["n"]
    if ri is not None:
        ri = np.asarray(ri, np.int64)
        assert len(ri) == 0 or (ri.min() >= 0 and ri.max() < t["m"])
        ent, row = _join(row, ri)
        col, val, m = col[ent], val[ent], len(ri)
    if ci is not None:
        ci = np.asarray(ci, np.int64)
        assert len(ci) == 0 or (ci.min() >= 0 and ci.max() < t["n"])
        ent, col = _join(col, ci)
        row, val, n = row[ent], val[ent], len(ci)
    return hr.from_coo(m, n, row, col, val)


def dense(t):
    d = np.zeros((t["m"], t["n"]))
    d[t["ir"], hr.cols_of(t)] = t["val"]
    return d


def rand_perm(n, seed):
    """cbg_rand_perm: the stable argsort of mix64(seed ^ (i * 0x9E3779B97F4A7C15))"""
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed) ^ (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)))
    return np.argsort(key, kind="stable").astype(np.int64)


def block_range(total, parts, idx):
    per = total // parts
    return idx * per, total if idx == parts - 1 else (idx + 1) * per


def load_imbalance(t, pr, pc):
    """SpParMat::LoadImbalance: the largest tile's nnz times the ranks over the global nnz"""
    row, col = t["ir"].astype(np.int64), hr.cols_of(t)
    most = 0
    for i in range(pr):
        r0, r1 = block_range(t["m"], pr, i)
        for j in range(pc):
            c0, c1 = block_range(t["n"], pc, j)
            most = max(most, int(np.sum((row >= r0) & (row < r1) & (col >= c0) & (col < c1))))
    return float(most) * (pr * pc) / len(row) if len(row) else 1.0


def nonisolated(t):
    """nonisov of RemoveIsolated (MCL.cpp:476-486): the vertices whose column sum is > 0"""
    return np.flatnonzero(hr.reduce_cols(t, "sum", 0.0) > 0).astype(np.int64)


def hipmcl_prepared(t, ps, remove_isolated=False, randpermute=False, seed=0x5EED):
    """HipMCL after RemoveIsolated and / or RandPermute -> (labels in t's numbering, iterations,
    [chaos], work_ids); a removed vertex is a cluster of its own"""
    ids = np.arange(t["n"], dtype=np.int64)
    w = t
    if remove_isolated:
        ids = nonisolated(w)
        w = spref(w, ids, ids)
    if randpermute:
        p = rand_perm(w["n"], seed)
        w = spref(w, p, p)
        ids = ids[p]
    lab, it, ch, _ = hr.hipmcl(w, *ps)
    full = np.full(t["n"], -1, np.int64)
    full[ids] = lab
    gone = np.flatnonzero(full < 0)
    full[gone] = (lab.max() + 1 if len(lab) else 0) + np.arange(len(gone))
    return hr.canonical(full), it, ch, ids


# ---------------------------------------------------------------------------
# test matrices and index vectors
# ---------------------------------------------------------------------------
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]


def main_tile(seed=7, m=301, n=257):
    """empty rows and columns, a column that holds every row but the empty ones (19), explicit
    +0.0, -0.0, inf and a NaN with a payload"""
    rng = np.random.default_rng(seed)
    dead_rows, dead_cols = [0, 5, 150, m - 1], [0, 3, 128, n - 1]
    live = np.setdiff1d(np.arange(m), dead_rows)
    row, col = [], []
    for j in np.setdiff1d(np.arange(n), dead_cols):
        r = live if j == 19 else rng.choice(live, int(rng.integers(1, 24)), replace=False)
        row.append(r)
        col.append(np.full(len(r), j))
    row, col = np.concatenate(row), np.concatenate(col)
    val = rng.uniform(-1, 1, len(row))
    val[::11] = 0.0
    val[1::13] = -0.0
    val[2::17] = np.inf
    val[3::19] = NAN_PAYLOAD
    return hr.from_coo(m, n, row, col, val)


def finite_tile(seed=9, m=301, n=257):
    """as main_tile without inf and NaN, -0.0 kept: for the comparison with the selection products"""
    t = main_tile(seed, m, n)
    v = t["val"].copy()
    bad = ~np.isfinite(v)
    v[bad] = 0.5
    return dict(t, val=v)


def index_cases(m, n, seed=3):
    """name -> (ri, ci); None: all"""
    rng = np.random.default_rng(seed)
    inc_r = np.sort(rng.choice(m, (2 * m) // 3, replace=False))
    inc_c = np.sort(rng.choice(n, n // 2, replace=False))
    return {
        "identity": (np.arange(m), np.arange(n)),
        "reversal": (np.arange(m)[::-1].copy(), np.arange(n)[::-1].copy()),
        "perm": (rng.permutation(m), rng.permutation(n)),
        "twoperm": (rng.permutation(m), rng.permutation(n)),
        "increasing": (inc_r, inc_c),
        "repeats": (rng.integers(0, m, m), rng.integers(0, n, n)),
        "repeats_tall": (rng.integers(0, m, m + 57), rng.integers(0, n, n - 20)),
        "rect": (rng.integers(0, m, 203), rng.integers(0, n, 97)),
        "rows_all": (None, rng.permutation(n)),
        "cols_all": (rng.permutation(m), None),
        "no_rows": (np.zeros(0, np.int64), np.arange(n)),
        "no_cols": (np.arange(m), np.zeros(0, np.int64)),
    }


def class_tile(bounds, m=8192, seed=11):
    """columns of length b - 1, b, b + 1 for every sort bound b, and 0, 1, 2; several of each"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2]
    for b in bounds:
        lens += [b - 1, b, b + 1]
    lens = lens + lens[::-1] + [max(bounds) * 2 + 5]
    row, col = [], []
    for j, ln in enumerate(lens):
        row.append(np.sort(rng.choice(m, ln, replace=False)))
        col.append(np.full(ln, j))
    row, col = np.concatenate(row), np.concatenate(col)
    return hr.from_coo(m, len(lens), row, col, rng.uniform(-1, 1, len(row))), lens


def golden_input(seed=21, m=60, n=50):
    """about 60 x 50 with empty rows and columns and signed values"""
    rng = np.random.default_rng(seed)
    keep = rng.random((m, n)) < 0.12
    keep[[0, 7, 33, m - 1], :] = False
    keep[:, [2, 25, n - 1]] = False
    row, col = np.nonzero(keep)
    val = np.round(rng.uniform(-4, 4, len(row)) * 64) / 64
    val[val == 0] = 0.25
    return hr.from_coo(m, n, row, col, val)


def golden_indices(m=60, n=50, seed=22):
    rng = np.random.default_rng(seed)
    p = rng.permutation(min(m, n))
    return {
        "symperm": (p, p),
        "twoperm": (rng.permutation(m), rng.permutation(n)),
        "increasing": (np.sort(rng.choice(m, 41, replace=False)), np.sort(rng.choice(n, 29, replace=False))),
        "rect": (rng.integers(0, m, 37), rng.integers(0, n, 23)),
    }


def golden_case(name):
    """(input, ri, ci) of a fixture.  The symmetric permutation runs on the square leading block
    of the input: the reference's symmetric path (one vector object for rows and columns,
    SpParMat.cpp:2141) multiplies by P and by P's transpose, which needs a square matrix."""
    t = golden_input()
    ri, ci = golden_indices(t["m"], t["n"])[name]
    if name == "symperm":
        k = min(t["m"], t["n"])
        t = spref(t, np.arange(k), np.arange(k))
    return t, ri, ci


def pad_isolated(t, at):
    """t with empty vertices inserted at the positions `at` of the new numbering"""
    n2 = t["n"] + len(at)
    keep = np.setdiff1d(np.arange(n2), np.asarray(at))
    return hr.from_coo(n2, n2, keep[t["ir"].astype(np.int64)], keep[hr.cols_of(t)], t["val"])


def pad_positions(n):
    return [0, 17, 40, n // 2, n + 4]
