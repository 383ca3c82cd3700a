#!/usr/bin/env python3
"""Batched betweenness centrality (cbg_grid_betwcent) on one GPU.

R-MAT (default scale 18, edge factor 16) symmetrised on the device (A + A^T through += of the
transpose), the first 2^K vertices with an out-edge as roots (the reference's rule,
betwcent_candidates), `--batch` roots at a time.  One run after a warm-up on the first batch.
Prints one JSON line and writes it to --out (default profiles/betwcent_s<scale>.json):

  teps              the reference's figure (BetwCent.cpp:221): nroots * nnz(A) / seconds
  split             cbg_last_betwcent_stats: host ms of the forward multiplies, the element-wise
                    ops, the backward multiplies, the dense ops, and the total
  ewise             the element-wise kernels over the whole run (cbg_last_ewise_stats, device ms):
                    bytes = 12 per entry of a and of out, 4 per entry of b (b's row ids, counted
                    whole: an upper bound of what the units' ranges touch; b's values are read on
                    hits under MULT only and are not counted), bytes / ms, and that as a fraction
                    of cbg_hbm_copy_bandwidth measured in this process.  The figure is a rough
                    gauge, neither an upper nor a lower bound of the traffic: b's row ids are counted
                    whole (too much), the re-reads of the binary searches and b's values under MULT
                    are not counted (too little), and the ms of a call span its one host readback
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load  # noqa: E402


class _Self:
    def bcast(self, comm, arr, root):
        pass

    def allgather(self, comm, data):
        return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--k4approx", type=int, default=9, help="2^K roots")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cbg = _load()
    cbg.lib().cbg_set_device(0)
    grid = cbg.CommGrid(0, 1, transport="host", host_comm=_Self())
    A = cbg.SpParMat.rmat(grid, a.scale, a.edgefactor)
    T = A.copy()
    T.Transpose()
    A += T  # symmetric: A is its own transpose
    T.tile.free()
    roots = cbg.betwcent_candidates(A, 1 << a.k4approx)
    copy_gbps = cbg.hbm_copy_bandwidth(1 << 30, 10)
    cbg.BetwCent(A, roots[:min(len(roots), a.batch)], a.batch, AT=A)  # warm-up: pools, code objects
    levels = []
    cbg.synchronize()
    t0 = time.perf_counter()
    bc = cbg.BetwCent(A, roots, a.batch, AT=A, on_level=lambda b, lv, nnz: levels.append((b, lv, nnz)))
    cbg.synchronize()
    sec = time.perf_counter() - t0
    st, ew = cbg.betwcent_stats(), cbg.ewise_stats()
    nbytes = 12 * (ew["entries_a"] + ew["entries_out"]) + 4 * ew["entries_b"]
    gbps = nbytes / (ew["ms"] * 1e-3) / 1e9 if ew["ms"] > 0 else 0.0
    res = dict(scale=a.scale, edgefactor=a.edgefactor, n=A.gn, nnz=A.tile.nnz, nroots=len(roots), batch=a.batch,
               seconds=sec, teps=len(roots) * A.tile.nnz / sec, split=st, levels=levels,
               ewise=dict(stats=ew, bytes=nbytes, gbps=gbps, copy_gbps=copy_gbps, fraction_of_copy=gbps / copy_gbps),
               ewise_bounds=cbg.ewise_bounds(), bc_max=float(bc.max()), bc_sum=float(bc.sum()))
    line = json.dumps(res)
    out = a.out or os.path.join(REPO, "profiles", f"betwcent_s{a.scale}.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
    grid.destroy()


if __name__ == "__main__":
    main()
