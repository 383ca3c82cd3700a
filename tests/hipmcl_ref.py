"""NumPy restatement of the HipMCL iteration (Applications/MCL.cpp:373-647) and the
test matrices of its tests.

A matrix is a DCSC dict (m, n, cp, jc, ir, val) of the WHOLE distributed matrix.
The multiply comes from helpers' CPU oracle, the pruning from mcl_ref, the connected
components are a union-find with the library's canonical labels (labels[v] = the
rank of v's component, components ordered by their smallest vertex).  Column sums
are np.sum's: bit-equal to the device only where the sums are exact (dyadic values);
tests/colsum_ref.py restates the device's own sum order, for inexact values."""
import numpy as np

import mcl_ref

DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny  # numeric_limits<double>::min()
EPS = 1e-4                           # MCL.cpp:55


def cols_of(t):
    """the column id of every entry"""
    return np.repeat(t["jc"].astype(np.int64), np.diff(t["cp"]))


def from_coo(m, n, row, col, val):
    """DCSC dict from distinct (row, col) pairs"""
    row, col, val = np.asarray(row, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float64)
    o = np.lexsort((row, col))
    row, col, val = row[o], col[o], val[o]
    jc, start = np.unique(col, return_index=True)
    return dict(m=int(m), n=int(n), cp=np.append(start, len(row)).astype(np.int64), jc=jc.astype(np.int32),
                ir=row.astype(np.int32), val=val)


def reduce_cols(t, what, identity=0.0):
    """SpParMat::Reduce(Column, ...): dense over the n columns; what: sum, max, sumsq, count"""
    out = np.full(t["n"], float(identity))
    for p, j in enumerate(t["jc"]):
        c = t["val"][t["cp"][p]:t["cp"][p + 1]]
        if what == "sum":
            out[j] = np.sum(c)
        elif what == "sumsq":
            out[j] = np.sum(c * c)
        elif what == "max":
            out[j] = max(float(identity), float(np.max(c)))
        else:
            out[j] = float(len(c))
    return out


def safe_inv(s):
    with np.errstate(divide="ignore"):
        return np.where(s == 0.0, DBL_MAX, 1.0 / s)


def make_col_stochastic(t):
    """MCL.cpp:390-395: v * (1 / sum), two roundings"""
    inv = safe_inv(reduce_cols(t, "sum"))
    with np.errstate(over="ignore", invalid="ignore"):
        return dict(t, val=t["val"] * inv[cols_of(t)])


def chaos(t):
    """MCL.cpp:408-421"""
    per = (reduce_cols(t, "max", 0.0) - reduce_cols(t, "sumsq")) * reduce_cols(t, "count")
    return float(max(0.0, np.max(per))) if len(per) else 0.0


def apply_pow(t, power):
    return dict(t, val=t["val"] * t["val"] if power == 2.0 else np.power(t["val"], power))


def inflate(t, power):
    """MCL.cpp:591-611 -> (matrix, chaos)"""
    s = make_col_stochastic(t)
    return make_col_stochastic(apply_pow(s, power)), chaos(s)


def remove_loops(t):
    col = cols_of(t)
    keep = t["ir"].astype(np.int64) != col
    return from_coo(t["m"], t["n"], t["ir"][keep], col[keep], t["val"][keep]), int(np.sum(~keep))


def add_loops(t, loopvals, replace_existing=False):
    """SpTuples::AddLoops (SpTuples.h:160-198): a loop on every vertex"""
    n = t["n"]
    lv = np.broadcast_to(np.asarray(loopvals, np.float64), (n,))
    col, row, val = cols_of(t), t["ir"].astype(np.int64), t["val"].copy()
    diag = row == col
    if replace_existing:
        val[diag] = lv[col[diag]]
    missing = np.setdiff1d(np.arange(n), col[diag])
    return from_coo(t["m"], n, np.concatenate([row, missing]), np.concatenate([col, missing]),
                    np.concatenate([val, lv[missing]]))


def adjust_loops(t):
    """MCL.cpp:464-474; the Apply at :469 acts on A: an empty column's loop stays DBL_MIN"""
    a, _ = remove_loops(t)
    colmax = reduce_cols(a, "max", DBL_MIN)
    a = dict(a, val=np.where(a["val"] == DBL_MIN, 1.0, a["val"]))
    return add_loops(a, colmax)


def components(n, rows, cols):
    """canonical labels of the undirected graph with edges (rows[i], cols[i])"""
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b in zip(np.asarray(rows, np.int64).tolist(), np.asarray(cols, np.int64).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)  # the root is the component's smallest vertex
    root = np.array([find(v) for v in range(n)], np.int64)
    rank = np.cumsum(root == np.arange(n)) - 1
    return rank[root] if n else np.zeros(0, np.int64)


def interpret(t):
    return components(t["n"], t["ir"], cols_of(t))


def canonical(labels):
    """any labelling -> the canonical one of the same partition"""
    labels = np.asarray(labels, np.int64)
    first = {}
    for v, l in enumerate(labels.tolist()):
        first.setdefault(l, v)
    root = np.array([first[l] for l in labels.tolist()], np.int64)
    rank = np.cumsum(root == np.arange(len(labels))) - 1
    return rank[root] if len(labels) else root


def printed_agrees(value, printed):
    """a chaos against the reference's printed one (setprecision(3)): half a unit of the
    third digit; below EPS the loop only asks "converged?", so only that must agree"""
    if printed < EPS:
        return value < EPS
    unit = 10.0 ** (np.floor(np.log10(printed)) - 2)
    return abs(value - printed) <= 0.5 * unit * (1 + 1e-6)


def load_golden(case):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"hipmcl_{case}.npz"),
                   allow_pickle=False)


def hipmcl(t, inflation=2.0, h=1e-4, S=1100, R=1400, q=0.9, preprune=None, eps=EPS, max_iterations=0, multiply=None,
           took=None):
    """HipMCL() (MCL.cpp:515-647) -> (labels, iterations, [chaos per iteration], final matrix)"""
    if multiply is None:
        from helpers import oracle_local
        multiply = oracle_local
    a = make_col_stochastic(adjust_loops(t))
    if preprune is None:
        preprune = len(a["ir"]) // a["n"] > max(S, R)
    if preprune:
        a = mcl_ref.mcl_prune_ref(a, h, S, R, q, took)
    c, it, seen = 1.0, 0, []
    while c > eps and (max_iterations == 0 or it < max_iterations):
        if took is not None:  # the longest column of any squared operand (see REF_SCAN_LIMIT)
            took["longest_column"] = max(took.get("longest_column", 0), int(np.diff(a["cp"]).max()))
        a = mcl_ref.mcl_prune_ref(multiply(a, dict(a)), h, S, R, q, took)
        a, c = inflate(a, inflation)
        seen.append(c)
        it += 1
    return interpret(a), it, seen, a


# ---------------------------------------------------------------------------
# test matrices
# ---------------------------------------------------------------------------
def loops_case(seed=3, n=40):
    """n x n: stored and missing diagonals, empty columns (0, 7, n - 1), a column whose loop
    is its first row (1), its last row (n - 2), an interior one (5), a column holding only
    its loop (9); dyadic values"""
    rng = np.random.default_rng(seed)
    row, col = [], []
    empty = {0, 7, n - 1}
    for j in range(n):
        if j in empty:
            continue
        k = int(rng.integers(1, 9))
        r = set(rng.choice(n, k, replace=False).tolist()) - {j}
        if j == 1:
            r = {j} | {x for x in r if x > j} | {n - 3}
        elif j == n - 2:
            r = {j} | {x for x in r if x < j} | {2}
        elif j == 5:
            r = {j, 0, n - 1}
        elif j == 9:
            r = {j}
        elif j % 3 == 0:
            r |= {j}
        if not r:
            r = {(j + 1) % n}
        for x in sorted(r):
            row.append(x)
            col.append(j)
    val = mcl_ref.dyadic(rng, len(row), 0.01, 0.9)
    return from_coo(n, n, row, col, val)


def planted(seed=1, n=96, groups=8):
    """8 dense groups of 12 with a few cross edges, symmetric, weights multiples of 2^-10,
    two isolated vertices and one vertex with only a loop"""
    rng = np.random.default_rng(seed)
    lone = {n - 1, n - 2, n - 3}
    w = {}
    size = n // groups
    for g in range(groups):
        mem = [v for v in range(g * size, (g + 1) * size) if v not in lone]
        for a in mem:
            for b in mem:
                if a < b and rng.random() < 0.85:
                    w[(a, b)] = float(rng.integers(512, 1024)) / 1024
    for _ in range(10):
        a, b = (int(x) for x in rng.integers(0, n - 3, 2))
        if a // size != b // size:
            w[(min(a, b), max(a, b))] = float(rng.integers(16, 64)) / 1024
    row = [a for a, b in w] + [b for a, b in w] + [n - 3]
    col = [b for a, b in w] + [a for a, b in w] + [n - 3]
    val = list(w.values()) * 2 + [0.5]
    return from_coo(n, n, row, col, val)


# The reference's HipMCL multiplies with LocalSpGEMMHash(..., sort = false) and merges with
# MultiwayMergeHash(..., sorted = false) (ParFriends.h:627, :668), so from the second
# iteration on the rows of a column are stored in hash-table order.  Its Dcsc::FillColInds
# (dcsc.cpp:1282-1342) looks up B's row ids in A's columns with std::set_intersection, which
# needs them ascending, whenever nzc(A tile) / nnz(B tile column) < THRESHOLD (4, SpDefs.h:126),
# and silently drops the products it misses.  With every column nonempty (the loops) a tile of
# the 128-vertex matrix has 128 nonempty columns on one rank and 64 on a 2 x 2 grid, so the
# reference multiplies correctly only while no squared operand has a column longer than
# 128 / 4 = 32 entries (one rank) or 64 / 4 = 16 (four ranks): the golden cases keep below 16,
# and the generator asserts it.  (Stars of 35 leaves have centre columns of 21 entries: the
# reference's 4-rank run of that graph lost 277 entries of the second square and ended in
# other clusters than its 1-rank run.)
REF_SCAN_LIMIT = 16


def hub(seed=2, n=128, leaves=24):
    """three stars (24 leaves each) joined by a path plus a 5-clique, directed weights (an
    edge is stored in one direction only, so Interpret's symmetrisation matters); 76
    columns are empty before the loops are added"""
    rng = np.random.default_rng(seed)
    e = {}
    centers = (0, 40, 80)
    for c in centers:
        for v in range(c + 1, c + 1 + leaves):
            e[(v, c) if v % 2 else (c, v)] = float(rng.integers(256, 1024)) / 1024
    path = [36, 37, 38, 39, 76, 77, 78, 79]
    chain = [0] + path[:4] + [40] + path[4:] + [80]
    for a, b in zip(chain[:-1], chain[1:]):
        e[(a, b)] = float(rng.integers(64, 256)) / 1024
    clique = list(range(120, 125))
    for a in clique:
        for b in clique:
            if a < b:
                e[(a, b) if (a + b) % 2 else (b, a)] = float(rng.integers(512, 1024)) / 1024
    row, col = [a for a, b in e], [b for a, b in e]
    return from_coo(n, n, row, col, list(e.values()))


CASES = {"planted": planted, "hub": hub}
# (inflation, h, S, R, q)
PARAM_SETS = ((2.0, 1e-4, 8, 10, 0.9), (1.7, 0.01, 0, 0, 0.0))
