"""Order-exact NumPy restatement of the device's column reductions: k_col_stats
(csrc/cbg_prune.hip), k_col_moments, k_col_moments_block, k_mom_combine and the three
passes of grid_inflate_device (csrc/cbg_mcl.hip).  This file is the statement of the
sum order; the GPU tests compare the device with it by bits on inexact values.

The order of a column's sum depends on its stored length alone:

  length <= 16    G = 16 lanes      (a 16-lane group)
  length <= 4096  G = 64 lanes      (a wave)
  longer          G = 256 lanes     (a block of four waves)

Lane l starts at +0.0 and adds entries l, l + G, l + 2G, ... one after another (an
entry that is not kept is skipped, not added as zero).  The lanes are combined by an
xor tree over distances 1, 2, 4, ...: neighbours first, (0,1), (2,3), then pairs of
pairs.  The block class runs the 64-lane tree in each of its four waves and adds the
wave sums as ((w0 + w1) + w2) + w3.  Products v * v are rounded before they are added
(no fused multiply-add).  The ranks of a grid column each reduce their own part by
these rules (the class from the part's length) and the parts are added in rank order.

Inputs must not hold a NaN, and no column's maximum may be a zero that occurs with
both signs: the maximum here is a plain maximum, the device folds with `>` and fmax,
which agree on everything else.

A matrix is a DCSC dict (m, n, cp, jc, ir, val), as in hipmcl_ref; `cuts` is an
optional ascending list of row ids at which a column is cut into the row blocks of a
grid column's ranks (cuts = [c] gives the blocks [0, c) and [c, m))."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny
GROUP_MAX, WAVE_MAX = 16, 4096  # cbg_mcl_moment_bounds
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 130, 4095, 4096, 4097, 4352, 4353, 8191)
PATTERNS = ("uniform", "wide", "normal")


def lanes_of(length):
    """the class of a column of `length` stored entries: its number of lanes"""
    return 16 if length <= GROUP_MAX else 64 if length <= WAVE_MAX else 256


def _tree(a, far_first=False):
    """xor tree over the lanes of a; lane 0 holds the result"""
    g = len(a)
    lane = np.arange(g)
    dist = [1 << k for k in range(g.bit_length() - 1)]
    for d in (reversed(dist) if far_first else dist):
        a = a + a[lane ^ d]
    return a[0]


def lane_sum(x, keep=None, lanes=None, far_first=False, wave_order=(0, 1, 2, 3)):
    """the sum of the elements x in device order.  keep: which elements take part (the
    class still comes from len(x)).  lanes, far_first, wave_order: other orders than the
    device's, for the tests that show the order matters"""
    x = np.asarray(x, np.float64)
    g = lanes_of(len(x)) if lanes is None else lanes
    rounds = -(-len(x) // g)
    pad = np.zeros(rounds * g)
    pad[:len(x)] = x
    use = np.zeros(rounds * g, bool)
    use[:len(x)] = True if keep is None else np.asarray(keep, bool)
    pad, use = pad.reshape(rounds, g), use.reshape(rounds, g)
    acc = np.zeros(g)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(rounds):
            acc = np.where(use[r], acc + pad[r], acc)
        if g <= 64:
            return float(_tree(acc, far_first))
        w = [_tree(acc[64 * k:64 * (k + 1)], far_first) for k in range(4)]
        a, b, c, d = (w[k] for k in wave_order)
        return float(((a + b) + c) + d)


def ordered_sum(values, keep=None):
    """sum of the kept values of one column (or one rank's part of it), device order"""
    return lane_sum(values, keep)


def ordered_sumsq(values, keep=None):
    v = np.asarray(values, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return lane_sum(v * v, keep)


def ordered_count(values, keep=None):
    return float(len(values) if keep is None else np.count_nonzero(keep))


def ordered_max(values, keep=None):
    """-inf for nothing kept"""
    v = np.asarray(values, np.float64)
    v = v if keep is None else v[np.asarray(keep, bool)]
    return float(np.max(v)) if len(v) else -np.inf


def combine_ranks(parts, what="sum"):
    """k_mom_preset and k_mom_combine: the ranks' parts in rank order; a rank without the
    column contributes 0.0 (-inf for the maximum)"""
    if what == "max":
        return float(max(parts))
    s = parts[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for p in parts[1:]:
            s = np.float64(s) + np.float64(p)
    return float(s)


_KINDS = {"sum": ordered_sum, "sumsq": ordered_sumsq, "count": ordered_count, "max": ordered_max}


def split_rows(rows, cuts):
    """slices of a column's (ascending) rows, one per row block"""
    at = [0] + [int(np.searchsorted(rows, c)) for c in (cuts or [])] + [len(rows)]
    return [slice(a, b) for a, b in zip(at[:-1], at[1:])]


def col_moment(values, rows, what, cuts=None, elems=None):
    """one kind of moment of a whole column: per row block, then in rank order.  elems:
    sum these elements instead of the values (the inflation's sum of w)"""
    x = values if elems is None else elems
    return combine_ranks([_KINDS[what](x[s]) for s in split_rows(rows, cuts)], what)


def _columns(t):
    for p, j in enumerate(t["jc"]):
        yield int(j), slice(int(t["cp"][p]), int(t["cp"][p + 1]))


def moments_ordered(t, cuts=None, elems=None):
    """dense (sum, sumsq, max, count) over the n columns: sums 0, max -inf, count 0 for a
    column nobody holds.  elems: the sum's elements where they are not the values"""
    n = t["n"]
    mom = dict(sum=np.zeros(n), sumsq=np.zeros(n), max=np.full(n, -np.inf), count=np.zeros(n))
    for j, s in _columns(t):
        v, r = t["val"][s], t["ir"][s]
        mom["sum"][j] = col_moment(v, r, "sum", cuts, None if elems is None else elems[s])
        for what in ("sumsq", "max", "count"):
            mom[what][j] = col_moment(v, r, what, cuts)
    return mom


def reduce_cols_ordered(t, what, identity=0.0, cuts=None):
    """SpParMat::Reduce(Column, ...) (k_mom_pick): the identity for an empty column, and
    folded into a maximum"""
    out = np.full(t["n"], float(identity))
    for j, s in _columns(t):
        x = col_moment(t["val"][s], t["ir"][s], what, cuts)
        out[j] = (x if x > identity else identity) if what == "max" else x
    return out


def col_stats_ordered(t, thr, strict):
    """Tile.col_stats: dense (cnt, sum) of the values kept under thr[column]"""
    cnt, tot = np.zeros(t["n"], np.int64), np.zeros(t["n"])
    for j, s in _columns(t):
        v = t["val"][s]
        keep = v > thr[j] if strict else ~(v < thr[j])
        cnt[j] = np.count_nonzero(keep)
        tot[j] = ordered_sum(v, keep)
    return cnt, tot


def safe_inv(s):
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(s == 0.0, DBL_MAX, 1.0 / s)


def cols_of(t):
    return np.repeat(t["jc"].astype(np.int64), np.diff(t["cp"]))


def make_col_stochastic_ordered(t, cuts=None):
    inv = safe_inv(moments_ordered(t, cuts)["sum"])
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return dict(t, val=t["val"] * inv[cols_of(t)])


def _chaos_of(mom):
    """k_chaos: folded from 0.0 with x > c ? x : c, so a NaN term is ignored"""
    with np.errstate(over="ignore", invalid="ignore"):
        mx = np.where(mom["max"] > 0.0, mom["max"], 0.0)
        x = (mx - mom["sumsq"]) * mom["count"]
    c = 0.0
    for v in x.tolist():
        c = v if v > c else c
    return c


def chaos_ordered(t, cuts=None):
    return _chaos_of(moments_ordered(t, cuts))


def inflate_ordered(t, power=2.0, pow_fn=None, cuts=None):
    """the three passes of grid_inflate_device -> (matrix, chaos).  pow_fn(v) -> w; for
    power 2 it is v * v"""
    if pow_fn is None:
        assert power == 2.0, "a power other than 2 needs the device's pow as pow_fn"
        pow_fn = lambda v: v * v  # noqa: E731
    col = cols_of(t)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        inv = safe_inv(moments_ordered(t, cuts)["sum"])                   # pass 1: column sums
        v = t["val"] * inv[col]                                            # pass 2: scale,
        w = pow_fn(v)                                                      #   pow,
        mom = moments_ordered(dict(t, val=v), cuts, elems=w)               #   moments of v, sum of w
        inv2 = safe_inv(mom["sum"])
        return dict(t, val=w * inv2[col]), _chaos_of(mom)                 # pass 3: scale


# ---------------------------------------------------------------------------
# test matrices: inexact values
# ---------------------------------------------------------------------------
def pattern_values(rng, pattern, n):
    if pattern == "uniform":
        return rng.uniform(0.0, 1.0, n)
    if pattern == "wide":
        return np.exp(rng.uniform(-30.0, 30.0, n))
    if pattern == "normal":  # mixed sign, cancellation
        return rng.standard_normal(n)
    if pattern == "dyadic":  # multiples of 2^-10: every sum is exact
        return rng.integers(-200, 600, n).astype(np.float64) / 1024.0
    raise ValueError(pattern)


def _from_columns(m, n, ids, rows, vals):
    cp = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int64)
    return dict(m=m, n=n, cp=cp, jc=np.asarray(ids, np.int32),
                ir=np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32),
                val=np.concatenate(vals).astype(np.float64) if vals else np.zeros(0))


_cache = {}


def inexact_case(pattern, per_length=16, m=16384):
    """per_length columns of every length of LENGTHS with values of `pattern` at random
    rows; every 16th column id is left empty.  Cached: do not modify"""
    key = (pattern, per_length, m)
    if key not in _cache:
        rng = np.random.default_rng(1000 + 7 * (PATTERNS + ("dyadic",)).index(pattern) + per_length)
        lens = [ln for ln in LENGTHS for _ in range(per_length)]
        n = len(lens) + len(lens) // 15 + 1
        ids = [j for j in range(n) if j % 16 != 5][:len(lens)]
        rows = [np.sort(rng.choice(m, ln, replace=False)) for ln in lens]
        vals = [pattern_values(rng, pattern, ln) for ln in lens]
        _cache[key] = _from_columns(m, n, ids, rows, vals)
    return _cache[key]


def column_lengths(t):
    """dense: the stored length of every column"""
    out = np.zeros(t["n"], np.int64)
    out[t["jc"]] = np.diff(t["cp"])
    return out


SPECIAL_LENGTHS = (3, 17, 4097)
SPECIAL_KINDS = ("inf", "cancel", "subnormal", "dbl_min", "neg_zero")


def special_values(kind, ln):
    if kind == "inf":        # sum inf, inverse 0: finite entries become 0, the inf NaN
        v = np.linspace(0.25, 0.75, ln)
        v[ln // 2] = np.inf
    elif kind == "cancel":   # integers: the sum is exactly 0 in any order, the inverse DBL_MAX
        v = np.where(np.arange(ln) % 2 == 0, -1.0, 1.0)
        v[:3] = (2.0, -1.0, -1.0)
        assert v.sum() == 0.0
    elif kind == "subnormal":  # the sum stays subnormal: its reciprocal overflows
        v = (1 + np.arange(ln) % 5) * 5e-324
    elif kind == "dbl_min":
        v = np.full(ln, DBL_MIN)
    elif kind == "neg_zero":  # documented: sums to +0.0
        v = np.full(ln, -0.0)
    else:
        raise ValueError(kind)
    return v.astype(np.float64)


def special_case(m=8192):
    """one column per (kind, length); column 2 and the last are empty"""
    if "special" not in _cache:
        rng = np.random.default_rng(77)
        cases = [(k, ln) for k in SPECIAL_KINDS for ln in SPECIAL_LENGTHS]
        ids = [j for j in range(len(cases) + 1) if j != 2]
        rows = [np.sort(rng.choice(m, ln, replace=False)) for _, ln in cases]
        vals = [special_values(k, ln) for k, ln in cases]
        _cache["special"] = _from_columns(m, len(cases) + 2, ids, rows, vals), cases
    return _cache["special"]


# (entries in the upper row block, entries in the lower) of the split columns: the class
# bounds on either side, a column empty in one block
SPLITS = ((16, 17), (17, 16), (4096, 4097), (4097, 4096), (1, 8000), (8000, 1), (0, 30), (30, 0), (64, 65), (65, 64),
          (4096, 16), (15, 4353), (100, 200), (3, 2), (2500, 2600), (5000, 70))


def split_case(pattern="uniform", m=16500, repeat=2):
    """m x n with `repeat` columns per entry of SPLITS: that many entries above and below
    row m // 2 (the cut of a grid with two row blocks); every 9th column id is empty"""
    key = ("split", pattern, m, repeat)
    if key not in _cache:
        rng = np.random.default_rng(4242 + repeat)
        half = m // 2
        sp = [s for s in SPLITS for _ in range(repeat)]
        ids = [j for j in range(len(sp) + len(sp) // 8 + 2) if j % 9 != 4][:len(sp)]
        rows = [np.concatenate([np.sort(rng.choice(half, a, replace=False)),
                                half + np.sort(rng.choice(m - half, b, replace=False))]) for a, b in sp]
        vals = [pattern_values(rng, pattern, a + b) for a, b in sp]
        _cache[key] = _from_columns(m, ids[-1] + 2, ids, rows, vals)
    return _cache[key]
