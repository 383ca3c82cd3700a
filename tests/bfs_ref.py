"""Host restatement of the single-source breadth-first search (cbg_grid_bfs, include/cbg.h): the loop of
Applications/TopDownBFS.cpp:427-443 with SelectMaxSRing<bool,int64>, the direction rule of
DirOptBFS.cpp:364-365, 388, 409, the serial count of the entries a pull reads, and a Graph500-style
validator.  numpy only; the checker of the tests, never the product.

ORIENTATION: y = A x.  A stored A(i, j) is the edge j -> i, so column j of the DCSC dict lists what j
reaches.  Values are ignored."""
import numpy as np

import hipmcl_ref as hr


def csr_of(t):
    """rows of A: (ptr, cols) with the column ids of every row ascending"""
    col = hr.cols_of(t)
    row = t["ir"].astype(np.int64)
    o = np.lexsort((col, row))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=t["m"]))]).astype(np.int64)
    return ptr, col[o]


def col_lengths(t):
    ln = np.zeros(t["n"], np.int64)
    ln[t["jc"]] = np.diff(t["cp"])
    return ln


def spmspv_max(t, xind, xval=None):
    """y[i] = max over stored t(i, j), j in xind, of x[j] (x[j] = j without xval) -> (yind, yval)"""
    xind = np.asarray(xind, np.int64)
    xval = xind if xval is None else np.asarray(xval, np.int64)
    pos = {int(j): p for p, j in enumerate(t["jc"])}
    best = {}
    for j, v in zip(xind.tolist(), xval.tolist()):
        p = pos.get(j)
        if p is None:
            continue
        for i in t["ir"][t["cp"][p]:t["cp"][p + 1]].tolist():
            if i not in best or v > best[i]:
                best[i] = v
    yi = np.array(sorted(best), np.int64)
    return yi, np.array([best[i] for i in yi.tolist()], np.int64)


def pull_max(t, xind, skip=None):
    """the same product (xval = ids) by scanning every row of t downward -> (yind, yval, entries_read):
    entries a serial descending scan reads, the hit included; a row without a hit: its length"""
    ptr, cols = csr_of(t)
    inx = np.zeros(t["n"], bool)
    inx[np.asarray(xind, np.int64)] = True
    yi, yv, read = [], [], 0
    for i in range(t["m"]):
        if skip is not None and skip[i]:
            continue
        for x in range(ptr[i + 1] - 1, ptr[i] - 1, -1):
            read += 1
            if inx[cols[x]]:
                yi.append(i)
                yv.append(int(cols[x]))
                break
    return np.array(yi, np.int64), np.array(yv, np.int64), read


def cutoffs(t):
    nnz, n = len(t["ir"]), t["n"]
    return nnz // 20, (int(float(n) * float(n) / (float(nnz) * 12.0)) if nnz else 0)


def bfs(t, root, direction="auto", up_cutoff=None, down_cutoff=None):
    """-> dict(parents, levels, steps, trace, stats).  steps: one (level, 'd' | 'u', frontier, pred) per
    step, as on_level sees them; trace: their directions as a string.  parents[root] = root as
    DirOptBFS.cpp:371 sets it."""
    n = t["n"]
    ptr, cols = csr_of(t)
    ln = col_lengths(t)
    up, down = cutoffs(t)
    up = up if up_cutoff is None else up_cutoff
    down = down if down_cutoff is None else down_cutoff
    parents, levels = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    parents[root], levels[root] = root, 0
    front = np.array([root], np.int64)
    pulling = direction == "bottomup"
    last, steps, fronts = 0, [], []
    st = dict(levels=0, reached=1, edges=0, push_steps=0, pull_steps=0, push_units=0, pull_rows=0, pull_entries=0)
    lev = 0
    while len(front):
        lev += 1
        pred = int(ln[front].sum())
        if direction == "auto" and not pulling and pred > up and last < len(front):
            pulling = True
        steps.append((lev, "u" if pulling else "d", len(front), pred))
        fronts.append(front)
        st["edges"] += pred
        if pulling:
            st["pull_steps"] += 1
            inx = np.zeros(n, bool)
            inx[front] = True
            cand = np.full(n, -1, np.int64)
            for i in np.flatnonzero((parents < 0) & (np.diff(ptr) > 0)).tolist():
                st["pull_rows"] += 1
                for x in range(ptr[i + 1] - 1, ptr[i] - 1, -1):
                    st["pull_entries"] += 1
                    if inx[cols[x]]:
                        cand[i] = cols[x]
                        break
        else:
            st["push_steps"] += 1
            yi, yv = spmspv_max(t, front)
            cand = np.full(n, -1, np.int64)
            cand[yi] = yv
        new = np.flatnonzero((cand >= 0) & (parents < 0))
        parents[new], levels[new] = cand[new], lev
        last, front = len(front), new
        st["reached"] += len(new)
        if len(new):
            st["levels"] = lev
        if direction == "auto" and pulling and len(front) < down and last > len(front):
            pulling = False
    return dict(parents=parents, levels=levels, steps=steps, trace="".join(s[1] for s in steps), stats=st, fronts=fronts)


def units_of(t, front, C, blocks=1):
    """push units of a frontier: ceil(len / C) per frontier column, the column's entries split over
    `blocks` row blocks of t["m"] // blocks rows (the last longer), every block's part counted alone"""
    total = 0
    per = t["m"] // blocks
    pos = {int(j): p for p, j in enumerate(t["jc"])}
    for j in np.asarray(front).tolist():
        p = pos.get(int(j))
        if p is None:
            continue
        rows = t["ir"][t["cp"][p]:t["cp"][p + 1]].astype(np.int64)
        blk = np.minimum(rows // per, blocks - 1) if per else np.full(len(rows), blocks - 1)
        total += int(sum(-(-c // C) for c in np.bincount(blk, minlength=blocks).tolist()))
    return total


def validate(t, root, parents, levels):
    """the Graph500 rules -> None, or the first violation as a string"""
    n = t["n"]
    parents, levels = np.asarray(parents, np.int64), np.asarray(levels, np.int64)
    if parents[root] != root or levels[root] != 0:
        return "the root is not its own parent at level 0"
    reached = parents >= 0
    if np.any(reached != (levels >= 0)):
        return "parents and levels disagree on what is reached"
    row, col = t["ir"].astype(np.int64), hr.cols_of(t)  # edge col -> row
    stored = set(zip(col.tolist(), row.tolist()))
    for v in np.flatnonzero(reached).tolist():
        if v == root:
            continue
        u = int(parents[v])
        if not (0 <= u < n) or (u, v) not in stored:
            return f"vertex {v}: no stored edge from its parent {u}"
        if levels[u] < 0 or levels[v] != levels[u] + 1:
            return f"vertex {v}: level {levels[v]} is not its parent's level {levels[u]} plus one"
    bad = reached[col] & ~reached[row]
    if np.any(bad):
        k = int(np.flatnonzero(bad)[0])
        return f"edge {col[k]} -> {row[k]} leaves the reached set"
    both = reached[col] & reached[row]
    far = both & (levels[row] > levels[col] + 1)
    if np.any(far):
        k = int(np.flatnonzero(far)[0])
        return f"edge {col[k]} -> {row[k]} spans more than one level"
    return None
