"""Restatements for the element-wise tile op and batched betweenness centrality.

ewise(a, b, op)    cbg_tile_ewise on DCSC dicts (m, n, cp, jc, ir, val), NumPy.
ewise_classes      the matching class of every work unit of cbg_tile_ewise, from its two bounds.
brandes(...)       Brandes betweenness centrality in exact rationals (fractions.Fraction):
                   A(i, j) stored = an edge i -> j, loops dropped, no halving, the source
                   excluded; bc sums the dependencies of the given roots.  With it the depth
                   and the shortest-path counts of every root, and the level sizes per batch.
"""
from fractions import Fraction

import numpy as np

import hipmcl_ref as hr

MULT, FIRST, EXCLUDE = 0, 1, 2


def _keys(t):
    return hr.cols_of(t) * np.int64(max(t["m"], 1)) + t["ir"].astype(np.int64)


def empty(m, n):
    return dict(m=int(m), n=int(n), cp=np.zeros(1, np.int64), jc=np.zeros(0, np.int32), ir=np.zeros(0, np.int32),
                val=np.zeros(0, np.float64))


def ewise(a, b, op):
    """b None: the empty tile.  MULT: a * b where both store; FIRST: a where both store;
    EXCLUDE: a where b does not store.  Values of FIRST / EXCLUDE are a's, untouched."""
    ka = _keys(a)
    if b is None or len(b["ir"]) == 0:
        hit, at = np.zeros(len(ka), bool), np.zeros(len(ka), np.int64)
    else:
        kb = _keys(b)  # ascending: columns ascending, rows ascending in a column
        at = np.minimum(np.searchsorted(kb, ka), len(kb) - 1)
        hit = kb[at] == ka
    keep = ~hit if op == EXCLUDE else hit
    val = a["val"][keep]
    if op == MULT:
        with np.errstate(invalid="ignore", over="ignore"):
            val = val * b["val"][at[keep]] if keep.any() else val
    col = hr.cols_of(a)[keep]
    jc, start = np.unique(col, return_index=True)
    return dict(m=a["m"], n=a["n"], cp=np.append(start, len(col)).astype(np.int64), jc=jc.astype(np.int32),
                ir=a["ir"][keep], val=val)


def ewise_classes(a, b, chunk, lds):
    """(units, units with no range of b, matched in LDS, matched in global memory)"""
    out = [0, 0, 0, 0]
    bpos = {int(j): p for p, j in enumerate(b["jc"])}
    for p, j in enumerate(a["jc"]):
        rows = a["ir"][a["cp"][p]:a["cp"][p + 1]].astype(np.int64)
        q = bpos.get(int(j))
        brows = b["ir"][b["cp"][q]:b["cp"][q + 1]].astype(np.int64) if q is not None else np.zeros(0, np.int64)
        for x in range(0, len(rows), chunk):
            c = rows[x:x + chunk]
            ln = int(np.searchsorted(brows, c[-1] + 1) - np.searchsorted(brows, c[0]))
            out[0] += 1
            out[1 if ln == 0 else 2 if ln <= lds else 3] += 1
    return tuple(out)


# ---------------------------------------------------------------------------
# exact Brandes
# ---------------------------------------------------------------------------
def out_neighbours(t):
    """adjacency lists of the graph whose edges i -> j are the stored A(i, j), loops dropped"""
    adj = [[] for _ in range(t["n"])]
    for i, j in zip(t["ir"].tolist(), hr.cols_of(t).tolist()):
        if i != j:
            adj[i].append(j)
    return adj


def brandes(t, roots, batch=None):
    """-> dict(bc: Fractions per vertex, depth: per root the deepest level reached, sigma_max:
    the largest shortest-path count, levels: per batch the sizes of the fringes the forward
    sweep sees, level 1 first (the neighbours of the batch's roots), sigma: per root the number
    of shortest paths to every vertex (0: not reached))"""
    n = t["n"]
    adj = out_neighbours(t)
    bc = [Fraction(0)] * n
    depth, sigma_max, per_root_levels, sigmas = [], 1, [], []
    for s in roots:
        dist = [-1] * n
        sigma = [0] * n
        dist[s], sigma[s] = 0, 1
        order, frontier, sizes = [], [s], []
        while frontier:
            order.append(frontier)
            nxt = []
            for v in frontier:
                for w in adj[v]:
                    if dist[w] < 0:
                        dist[w] = dist[v] + 1
                        nxt.append(w)
                    if dist[w] == dist[v] + 1:
                        sigma[w] += sigma[v]
            frontier = nxt
            if nxt:
                sizes.append(len(nxt))
        delta = [Fraction(0)] * n
        for level in reversed(order):
            for v in level:
                for w in adj[v]:
                    if dist[w] == dist[v] + 1:
                        delta[v] += Fraction(sigma[v], sigma[w]) * (1 + delta[w])
                if v != s:
                    bc[v] += delta[v]
        depth.append(len(order) - 1)
        sigma_max = max(sigma_max, max(sigma))
        per_root_levels.append(sizes)
        sigmas.append(sigma)
    batch = len(roots) if batch is None else batch
    levels = []
    for b0 in range(0, len(roots), batch):
        group = per_root_levels[b0:b0 + batch]
        deepest = max((len(g) for g in group), default=0)
        levels.append([sum(g[k] for g in group if len(g) > k) for k in range(deepest)])
    return dict(bc=bc, depth=depth, sigma_max=sigma_max, levels=levels, sigma=sigmas)


def max_degree(t):
    adj = out_neighbours(t)
    indeg = [0] * t["n"]
    for v in range(t["n"]):
        for w in adj[v]:
            indeg[w] += 1
    return max([len(a) for a in adj] + indeg + [0])


def bound_factor(depth, degree, nroots, batches):
    """K of |bc_got - bc_exact| <= K * 2^-52 * (bc_exact + nroots): the roundings on the longest chain"""
    return depth * (degree + 4) + nroots + batches + 2
