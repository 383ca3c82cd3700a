#!/usr/bin/env python3
"""Sparse indexing A(ri, ci) on one GPU: the direct path (SubsRef: cbg_grid_spref) against
the reference's route, two SUMMA products P * A * Q with selection matrices.

R-MAT (default scale 20, edge factor 16) on a 1 x 1 grid, two indexings:
  permute     A(p, p), p = rand_perm(n, 1): every column is sorted
  nonisolated A(nonisov, nonisov): ri strictly increasing, nothing is sorted
One warm-up, then the median of --reps runs of each route.  P and Q are uploaded before the
clock starts.  The route of the reference runs through Mult_AnXBn_DoubleBuff unchanged.
For the direct path the stage times of cbg_last_spref_stats are reported, and its bytes over
its time as a fraction of cbg_hbm_copy_bandwidth measured in this process: 12 B read and
12 B written per entry for the column stage (entries in), for the row stage (entries out)
and for every sort pass made (entries out; the wave and LDS classes sort a column in one
pass in place, `sort_passes` is 1 when a column was sorted and 0 otherwise; the columns of
the radix class, counted in `sorted_radix`, take one pass per 8-bit digit on top).
Both routes must give the same tile (digests compared).  Prints one JSON line and writes it
to --out (default profiles/spref_s<scale>.json).
"""
import argparse
import json
import os
import statistics
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


def selection(cbg, grid, idx, extent, rows):
    """P (rows=True: len(idx) x extent, P(i, idx[i]) = 1) or Q (extent x len(idx), Q(idx[j], j) = 1)"""
    k = len(idx)
    if rows:
        order = np.argsort(idx, kind="stable")
        jc, start = np.unique(idx[order], return_index=True)
        d = dict(m=k, n=extent, cp=np.append(start, k).astype(np.int64), jc=jc.astype(np.int32),
                 ir=order.astype(np.int32), val=np.ones(k))
    else:
        d = dict(m=extent, n=k, cp=np.arange(k + 1, dtype=np.int64), jc=np.arange(k, dtype=np.int32),
                 ir=idx.astype(np.int32), val=np.ones(k))
    return cbg.SpParMat(cbg.Tile.from_dict(d), grid, d["m"], d["n"])


def timed(fn, reps, cbg):
    out = []
    for i in range(reps + 1):
        cbg.synchronize()
        t0 = time.perf_counter()
        r = fn()
        cbg.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if i:
            out.append((ms, r))
    ms = [x[0] for x in out]
    return statistics.median(ms), min(ms), max(ms), out[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cbg = _load()
    cbg.lib().cbg_set_device(0)
    grid = cbg.CommGrid(0, 1, transport="host", host_comm=_Self())
    A = cbg.SpParMat.rmat(grid, a.scale, a.edgefactor)
    n = A.gn
    copy_gbps = cbg.hbm_copy_bandwidth(1 << 30, 10)
    res = dict(scale=a.scale, edgefactor=a.edgefactor, n=n, nnz=A.tile.nnz, reps=a.reps, copy_gbps=copy_gbps,
               sort_bounds=cbg.spref_sort_bounds(), cases={})
    _, nonisov = cbg.RemoveIsolated(A)
    for name, idx in (("permute", cbg.rand_perm(n, 1)), ("nonisolated", nonisov)):
        stats = []

        def direct():
            B = A.SubsRef(idx, idx)
            stats.append(cbg.spref_stats())
            return B

        med, lo, hi, B = timed(direct, a.reps, cbg)
        st = stats[-1]
        stage = {k: statistics.median(s[k] for s in stats[1:]) for k in ("ms_col", "ms_row", "ms_sort")}
        sort_passes = 1 if st["sorted_wave"] + st["sorted_lds"] + st["sorted_radix"] else 0
        nbytes = 24 * (st["entries_in"] + st["entries_out"] + sort_passes * st["entries_out"])
        P, Q = selection(cbg, grid, idx, n, True), selection(cbg, grid, idx, n, False)

        def triple():
            PA = cbg.Mult_AnXBn_DoubleBuff(P, A)
            C = cbg.Mult_AnXBn_DoubleBuff(PA, Q)
            PA.tile.free()
            return C

        tmed, tlo, thi, C = timed(triple, a.reps, cbg)
        db, dc = B.tile.digest(), C.tile.digest()
        same = all(db[k] == dc[k] for k in ("nnz", "nzc", "hs", "hv", "unsorted"))
        res["cases"][name] = dict(
            nri=len(idx), direct_ms=med, direct_ms_min=lo, direct_ms_max=hi, stage_ms=stage, stats=st,
            sort_passes=sort_passes, bytes=nbytes, gbps=nbytes / (med * 1e-3) / 1e9,
            fraction_of_copy=nbytes / (med * 1e-3) / 1e9 / copy_gbps, triple_product_ms=tmed, triple_product_ms_min=tlo,
            triple_product_ms_max=thi, speedup=tmed / med, same_result=same, unsorted=db["unsorted"])
        for t in (B, C, P, Q):
            t.tile.free()
    line = json.dumps(res)
    out = a.out or os.path.join(REPO, "profiles", f"spref_s{a.scale}.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
    grid.destroy()


if __name__ == "__main__":
    main()
