#!/usr/bin/env python3
"""Single-source breadth-first search (cbg_grid_bfs) on one GPU, Graph500 style.

R-MAT (default scale 18, edge factor 16) symmetrised on the device (A + A^T through += of the
transpose), 64 seeded roots of nonzero degree, the local transpose made once, every root searched
under the reference's direction rule ("auto") and top-down only.  Every auto tree is validated on
the host by the Graph500 rules, and the top-down tree has to be the same bits.  Writes one JSON
line to --out (default profiles/bfs_s<scale>.json) and prints its summary; per mode:

  seconds, teps     per root; teps = edges / seconds with edges the summed degrees of the reached
                    vertices (TopDownBFS.cpp:448-452; the symmetrised matrix stores every undirected
                    edge twice, and so does this count)
  hmean_teps        the harmonic mean of the roots' teps, as the reference prints it (TopDownBFS.cpp:512-520)
  share             push, pull, update, communication as fractions of the summed totals (host ms of
                    cbg_last_bfs_stats; the rest is the agreements and the callback)
  one_root          the first root's steps: level, direction, frontier, pred, and the host ms between
                    the callbacks of consecutive steps
  traffic           bytes each direction must touch against the device copy bandwidth measured in this
                    process: push 4 B per traversed entry (its row id; the atomic comes on top), pull 4 B
                    per entry read plus the frontier bitmap once per step; GB/s over the push / pull ms
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load  # noqa: E402


class _Self:
    def bcast(self, comm, arr, root):
        pass

    def allgather(self, comm, data):
        return data


def validate(row, col, root, parents, levels):
    """the Graph500 rules, vectorised; (row, col) the stored entries: an edge col -> row"""
    reached = parents >= 0
    assert parents[root] == root and levels[root] == 0, "the root is not its own parent at level 0"
    assert np.array_equal(reached, levels >= 0), "parents and levels disagree"
    v = np.flatnonzero(reached)
    v = v[v != root]
    assert np.all(levels[parents[v]] >= 0) and np.all(levels[v] == levels[parents[v]] + 1), "a level is not the parent's plus one"
    fwd = reached[col]
    assert np.all(reached[row[fwd]]), "an edge leaves the reached set"
    assert np.all(levels[row[fwd]] <= levels[col[fwd]] + 1), "an edge spans more than one level"
    tree = (parents[row] == col) & (row != root)
    assert int(tree.sum()) == len(v), "a parent's edge is not stored"


def hmean(x):
    return len(x) / float(np.sum(1.0 / np.asarray(x)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--roots", type=int, default=64)
    ap.add_argument("--seed", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cbg = _load()
    cbg.lib().cbg_set_device(0)
    grid = cbg.CommGrid(0, 1, transport="host", host_comm=_Self())
    A = cbg.SpParMat.rmat(grid, a.scale, a.edgefactor)
    T = A.copy()
    T.Transpose()
    A += T  # symmetric; an entry stored both ways is stored once
    T.tile.free()
    At = A.tile.transpose()  # once for all the roots
    h = A.tile.to_host()
    row, col = h["ir"].astype(np.int64), np.repeat(h["jc"].astype(np.int64), np.diff(h["cp"]))
    deg = np.zeros(A.gn, np.int64)
    deg[h["jc"]] = np.diff(h["cp"])
    roots = np.random.default_rng(a.seed).choice(np.flatnonzero(deg > 0), a.roots, replace=False)
    copy_gbps = cbg.hbm_copy_bandwidth(1 << 30, 10)
    cbg.BFS(A, int(roots[0]), "auto", At=At)  # warm-up: pools, code objects
    cbg.BFS(A, int(roots[0]), "topdown")
    res = dict(scale=a.scale, edgefactor=a.edgefactor, n=A.gn, nnz=A.tile.nnz, nroots=len(roots), seed=a.seed,
               bounds=cbg.bfs_bounds(), copy_gbps=copy_gbps, modes={})
    trees = {}
    for mode in ("auto", "topdown"):
        secs, teps, edges, traces, tot = [], [], [], [], {}
        push_entries = pull_entries = pull_steps = 0
        one = None
        for k, root in enumerate(roots.tolist()):
            steps = []
            cbg.synchronize()
            t0 = time.perf_counter()
            parents, levels = cbg.BFS(A, root, mode, At=At, on_level=lambda *s: steps.append(s + (time.perf_counter(),)))
            sec = time.perf_counter() - t0
            st = cbg.bfs_stats()
            # checked after the timed loop: host work between two searches lets the device clock down
            trees.setdefault(root, {})[mode] = (parents.copy(), levels.copy())
            secs.append(sec)
            edges.append(st["edges"])
            teps.append(st["edges"] / sec)
            traces.append("".join(s[1] for s in steps))
            for key, val in st.items():
                tot[key] = tot.get(key, 0) + val
            push_entries += sum(s[3] for s in steps if s[1] == "d")
            pull_entries += st["pull_entries"]
            pull_steps += st["pull_steps"]
            if k == 0:
                ends = [s[4] for s in steps[1:]] + [t0 + sec]
                one = dict(root=root, steps=[dict(level=s[0], direction=s[1], frontier=s[2], pred=s[3], ms=(e - s[4]) * 1e3)
                                             for s, e in zip(steps, ends)])
        push_bytes, pull_bytes = 4 * push_entries, 4 * pull_entries + pull_steps * (A.gn // 8)
        push_gbps = push_bytes / (tot["ms_push"] * 1e-3) / 1e9 if tot["ms_push"] > 0 else 0.0
        pull_gbps = pull_bytes / (tot["ms_pull"] * 1e-3) / 1e9 if tot["ms_pull"] > 0 else 0.0
        res["modes"][mode] = dict(
            seconds=secs, teps=teps, edges=edges, traces=traces, hmean_teps=hmean(teps), mean_seconds=float(np.mean(secs)),
            totals=tot, share={k: tot["ms_" + k] / tot["ms_total"] for k in ("push", "pull", "update", "comm")}, one_root=one,
            traffic=dict(push_bytes=push_bytes, pull_bytes=pull_bytes, push_gbps=push_gbps, pull_gbps=pull_gbps,
                         push_fraction_of_copy=push_gbps / copy_gbps, pull_fraction_of_copy=pull_gbps / copy_gbps))
    for root, t in trees.items():
        validate(row, col, root, *t["auto"])
        assert np.array_equal(t["auto"][0], t["topdown"][0]) and np.array_equal(t["auto"][1], t["topdown"][1]), root
    res["validated"] = len(trees)
    line = json.dumps(res)
    out = a.out or os.path.join(REPO, "profiles", f"bfs_s{a.scale}.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    print(json.dumps({m: dict(hmean_teps=v["hmean_teps"], mean_seconds=v["mean_seconds"], share=v["share"],
                              traffic=v["traffic"], first_trace=v["traces"][0]) for m, v in res["modes"].items()}))
    grid.destroy()


if __name__ == "__main__":
    main()
