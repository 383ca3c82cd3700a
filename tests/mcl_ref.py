"""NumPy restatement of MCLPruneRecoverySelect (ParFriends.h:186-353) and the test
matrices of the pruning tests.

A matrix is a DCSC dict (m, n, cp, jc, ir, val) of the WHOLE distributed matrix:
every decision is per global column.  With h = hardThreshold, S = selectNum,
R = recoverNum, q = recoverPct:

  1. cnt0 = #{v > h}, sum0 = sum{v : v > h}, all = nnz of the column; thr = h.
  2. recovery: columns with cnt0 < R, all > cnt0 and sum0 < q get thr = kth(R).
  3. if S > 0: the columns outside step 2 with cnt0 > S get thr = kth(S); if also
     R > 0, those of them with cnt1 = #{!(v < thr)} < R and sum1 < q get thr = kth(R).
  4. keep v iff !(v < thr); emptied columns leave jc.

kth(k) is the k-th largest value of the unpruned column, duplicates counted, the
smallest value when the column has fewer than k entries.  All test values are
multiples of 2^-10 bounded so that every column sum is exact in double: the sums
compare against q exactly whatever their order, and results are compared by bits.
NaN values are outside the restatement (unspecified)."""
import numpy as np

BRANCHES = ("recovery", "selection", "recovery_after_selection", "fewer_than_k", "ties_at_kth", "equal_to_h",
            "emptied_by_h", "all_negative")


def kth_largest(col, k):
    s = np.sort(np.asarray(col, np.float64))[::-1]
    return float(s[min(int(k), len(s)) - 1]) + 0.0  # a zero is +0.0, as the library returns it


def mcl_thresholds(t, h, S, R, q):
    """per nonempty column: the final threshold; and the branches each column took"""
    cp, val = t["cp"], t["val"]
    nzc = len(t["jc"])
    cols = [val[cp[p]:cp[p + 1]] for p in range(nzc)]
    took = {b: set() for b in BRANCHES}
    thr = np.full(nzc, float(h))
    cnt0 = np.array([int(np.sum(c > h)) for c in cols], np.int64)
    sum0 = np.array([float(np.sum(c[c > h])) for c in cols])
    alln = np.array([len(c) for c in cols], np.int64)

    def select(p, k, why):
        thr[p] = kth_largest(cols[p], k)
        took[why].add(p)
        if len(cols[p]) < k:
            took["fewer_than_k"].add(p)
        elif int(np.sum(~(cols[p] < thr[p]))) > k:
            took["ties_at_kth"].add(p)

    rec = (cnt0 < R) & (alln > cnt0) & (sum0 < q)
    for p in np.flatnonzero(rec):
        select(p, R, "recovery")
    if S > 0:
        sel = ~rec & (cnt0 > S)
        for p in np.flatnonzero(sel):
            select(p, S, "selection")
        if R > 0:
            for p in np.flatnonzero(sel):
                kept = cols[p][~(cols[p] < thr[p])]
                if len(kept) < R and float(np.sum(kept)) < q:
                    select(p, R, "recovery_after_selection")
    for p in range(nzc):
        c = cols[p]
        if thr[p] == h and np.any(c == h):
            took["equal_to_h"].add(p)  # counted out in step 1, kept in step 4
        if not np.any(~(c < thr[p])):
            took["emptied_by_h"].add(p)
        if np.all(c < 0):
            took["all_negative"].add(p)
    return thr, took


def prune_columns(t, thr):
    """step 4 with one threshold per NONEMPTY column of t"""
    cnt = np.diff(t["cp"])
    keep = ~(t["val"] < np.repeat(thr, cnt))
    pcol = np.repeat(np.arange(len(cnt)), cnt)[keep]
    kept = np.bincount(pcol, minlength=len(cnt)).astype(np.int64)
    ne = kept > 0
    return dict(m=t["m"], n=t["n"], cp=np.concatenate([[0], np.cumsum(kept[ne])]).astype(np.int64),
                jc=t["jc"][ne].astype(np.int32), ir=t["ir"][keep].astype(np.int32),
                val=t["val"][keep].astype(np.float64))


def mcl_prune_ref(t, h, S, R, q, took=None):
    if h <= 0 and S <= 0 and R <= 0 and q <= 0:  # the library's rule: no pruning at all
        return dict(t)
    thr, tk = mcl_thresholds(t, h, S, R, q)
    if took is not None:
        for b in BRANCHES:
            took.setdefault(b, set()).update(tk[b])
    return prune_columns(t, thr)


def col_stats_ref(t, thr, strict):
    """dense (cnt, sum) over the n columns under thr[column]"""
    cnt = np.zeros(t["n"], np.int64)
    tot = np.zeros(t["n"], np.float64)
    for p, j in enumerate(t["jc"]):
        c = t["val"][t["cp"][p]:t["cp"][p + 1]]
        k = c > thr[j] if strict else ~(c < thr[j])
        cnt[j] = int(np.sum(k))
        tot[j] = float(np.sum(c[k]))
    return cnt, tot


# ---------------------------------------------------------------------------
# test matrices
# ---------------------------------------------------------------------------
H, Q, S_NUM, R_NUM = 0.125, 0.75, 3, 5  # the pruning tests' parameters (S = 3, R = 5)
PARAM_SETS = ((H, 0, 0, 0.0), (H, S_NUM, 0, 0.0), (H, S_NUM, R_NUM, Q), (0.0, 0, R_NUM, Q))


def dyadic(rng, n, lo=-0.2, hi=0.6):
    """n multiples of 2^-10 in [lo, hi)"""
    return rng.integers(int(lo * 1024), int(hi * 1024), n).astype(np.float64) / 1024.0


def branch_columns():
    """columns (values only) that take each branch under (H, S_NUM, R_NUM, Q) or (H, S_NUM, 0, 0)"""
    u = 1.0 / 1024
    return [
        [0.25, 0.1875, 0.0625, 0.03125, 0.0625 + u, 0.015625, 0.046875, 0.0078125],   # recovery (2 above h of 8)
        [0.5, 0.5 - u, 0.25, 0.25 - u, 0.1875, 0.15625, 0.140625, 0.13],              # selection, top 3 sum >= q
        [0.24, 0.23, 0.22, 0.21, 0.2, 0.19, 0.18, 0.17, 0.01],                         # rounded below
        [0.25, 0.0625, 0.03125],                                                       # recovery, fewer than R
        [0.5, 0.375, 0.25, 0.25, 0.25, 0.1875, 0.15625, 0.0625],                       # ties across the 3rd place
        [0.5, 0.5, 0.375, H, H, 0.0625],                                               # values equal to h (kept: thr stays h)
        [0.0625, 0.03125, 0.015625],                                                   # emptied when R = 0
        [-0.25, -0.125, -0.5, -0.0625],                                                # all negative
        [0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2],                                           # all equal
        [0.0, -0.0, 0.25, 0.375, 0.5, 0.625],                                          # both zeros
        [0.3],                                                                          # one entry
    ]


def _round(cols):
    return [np.round(np.asarray(c, np.float64) * 1024) / 1024 for c in cols]


def build_tile(rng, m, n, col_vals, where=None):
    """DCSC dict with the given columns' values at random distinct rows; `where`
    places column i at id where[i] (default: spread over n with gaps)"""
    k = len(col_vals)
    ids = np.sort(rng.choice(n, k, replace=False)) if where is None else np.asarray(where)
    order = np.argsort(ids)
    cp, ir, val = [0], [], []
    for i in order:
        v = np.asarray(col_vals[i], np.float64)
        ir.append(np.sort(rng.choice(m, len(v), replace=False)).astype(np.int32))
        val.append(v)
        cp.append(cp[-1] + len(v))
    return dict(m=m, n=n, cp=np.asarray(cp, np.int64), jc=ids[order].astype(np.int32),
                ir=np.concatenate(ir) if ir else np.zeros(0, np.int32),
                val=np.concatenate(val) if val else np.zeros(0, np.float64))


def assert_all_branches(t, param_sets=PARAM_SETS):
    took = {}
    for (h, S, R, q) in param_sets:
        mcl_prune_ref(t, h, S, R, q, took)
    missing = [b for b in BRANCHES if not took.get(b)]
    assert not missing, f"branches that no column takes: {missing}"


def small_case(seed, m=64, n=48):
    """about 64 x 48: the branch columns plus random ones, some columns empty"""
    rng = np.random.default_rng(seed)
    cols = _round(branch_columns())
    for _ in range(n - len(cols) - 6):
        cols.append(dyadic(rng, int(rng.integers(1, 24))))
    t = build_tile(rng, m, n, cols)
    assert_all_branches(t)
    return t


def big_case(seed=5, m=32768, n=300, bounds=(512, 4096, 16384)):
    """32768 x 300: the branch columns, random short ones, and columns longer than every
    k-select class bound (so selection and recovery run in every kernel class)"""
    rng = np.random.default_rng(seed)
    cols = _round(branch_columns())
    for b in bounds:
        for ln in (b - 1, b, b + 1):
            cols.append(dyadic(rng, ln))
    cols.append(dyadic(rng, 30000))
    # a long column that recovery rescues: two values above h, thousands below
    cols.append(np.concatenate([[0.25, 0.1875], dyadic(rng, 20000, 0.0, 0.12)]))
    for _ in range(n - len(cols) - 20):
        cols.append(dyadic(rng, int(rng.integers(1, 200))))
    t = build_tile(rng, m, n, cols)
    assert_all_branches(t)
    return t


def dyadic_values(t, mod=8, denom=16):
    """R-MAT structure with exact values: (1 + (7 row + 13 col) % mod) / denom"""
    cnt = np.diff(t["cp"])
    col = np.repeat(t["jc"].astype(np.int64), cnt)
    v = (1 + (7 * t["ir"].astype(np.int64) + 13 * col) % mod).astype(np.float64) / denom
    return dict(t, val=v)


def multirank_case(seed=9, m=32768, n=300):
    """big_case plus, for grids with two row blocks, a column whose top entries all lie
    in the upper row block, one that is empty in the upper block and one empty in the lower"""
    rng = np.random.default_rng(seed)
    t = big_case(seed, m, n)
    free = np.setdiff1d(np.arange(n), t["jc"])
    half = m // 2
    extra = {
        int(free[0]): (np.concatenate([np.arange(0, 40, 2), half + np.arange(0, 90, 3)]),           # top 20 above the cut
                       np.concatenate([0.5 + np.arange(20) / 1024.0, 0.13 + np.arange(30) / 1024.0])),
        int(free[1]): (half + np.arange(5, 65, 2), dyadic(rng, 30, 0.0, 0.6)),                      # nothing in block 0
        int(free[len(free) // 2]): (np.arange(7, 57, 5), dyadic(rng, 10, 0.0, 0.6)),                # nothing in block 1
    }
    cnt = np.diff(t["cp"])
    col = np.concatenate([np.repeat(t["jc"].astype(np.int64), cnt)] + [np.full(len(r), j) for j, (r, _) in extra.items()])
    row = np.concatenate([t["ir"].astype(np.int64)] + [np.asarray(r, np.int64) for r, _ in extra.values()])
    val = np.concatenate([t["val"]] + [np.asarray(v, np.float64) for _, v in extra.values()])
    o = np.lexsort((row, col))
    col, row, val = col[o], row[o], val[o]
    jc, start = np.unique(col, return_index=True)
    out = dict(m=m, n=n, cp=np.append(start, len(row)).astype(np.int64), jc=jc.astype(np.int32), ir=row.astype(np.int32),
               val=val)
    assert_all_branches(out)
    return out
