#!/usr/bin/env python3
"""Cost of the Markov-clustering pruning next to the multiply it follows.

R-MAT (default scale 20, edge factor 16) with column-normalised values, squared
with MemEfficientSpGEMM_MCL at HipMCL's usual parameters (select 1100, recover
1400, recoverPct 0.9, hardThreshold 1e-4) on one GPU: one warm-up, then the median
of --reps runs.  Reports, per phase, the multiply's device ms and the prune's by
stage (statistics, k-select, compaction), the columns each k-select class ran, and
for the two streaming passes the achieved bytes/s as a fraction of
cbg_hbm_copy_bandwidth measured in the same process:
  statistics: 8 B per entry and pass (one pass, two where selection ran with recovery);
  compaction: 8 B per entry (count) + 12 B per entry read + 12 B per kept entry written.
The multiply accumulates its sums with floating-point LDS atomics, so with these
inexact values the low bits of C -- and with them a few near-tie pruning decisions --
differ from run to run.  The pruning itself is checked for repeatability on one fixed
unpruned product (two prunes, equal digests), and the phase independence of the whole
pruned product with exact values ((1 + (7 row + 13 col) % 8) / 16, every sum exact):
the digests for phases 1, the memory-chosen count and 4 must be equal.  Writes one JSON document (--out, default
profiles/mcl_bench_s<scale>.json) and prints it.

--iterate runs the whole HipMCL loop instead (AdjustLoops, MakeColStochastic, then the
pruned squaring and the fused inflation until chaos <= 1e-4) and writes
profiles/hipmcl_s<scale>.json: see iterate().
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


def run(cbg, A, B, phases, params, digest=True):
    """one pruned product, streamed: per-piece stage times and the order-free digest"""
    pieces, prev = [], dict(mult=0.0, stats=0.0, kselect=0.0, compact=0.0, ein=0, eout=0)
    acc = dict(nnz=0, hs=0, hv=0)

    def on_phase(p, off, t):
        ls, ms = cbg.last_stats(), cbg.mcl_stats()
        cur = dict(mult=ls["ms_symbolic"] + ls["ms_numeric"], stats=ms["ms"]["stats"], kselect=ms["ms"]["kselect"],
                   compact=ms["ms"]["compact"], ein=ms["entries_in"], eout=ms["entries_out"])
        pieces.append(dict(phase=p, col_offset=off, **{k: cur[k] - prev[k] for k in cur}))
        prev.update(cur)
        if digest:
            d = t.digest(0, off)
            acc["nnz"] += d["nnz"]
            acc["hs"] = (acc["hs"] + int(d["hs"], 16)) % (1 << 64)
            acc["hv"] = (acc["hv"] + int(d["hv"], 16)) % (1 << 64)

    t0 = time.perf_counter()
    cbg.MemEfficientSpGEMM_MCL(A, B, phases, *params, on_phase=on_phase)
    cbg.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return dict(wall_ms=wall, pieces=pieces, stats=cbg.mcl_stats(), plan=cbg.phase_plan(),
                digest=dict(nnz=acc["nnz"], hs="%016x" % acc["hs"], hv="%016x" % acc["hv"]))


def iterate(cbg, A, a):
    """--iterate: the whole HipMCL loop on the normalised R-MAT.  Per iteration the expand,
    prune and inflate ms and the nnz; for the inflation's three passes the achieved bytes/s
    (pass 1 reads 8 B per entry, passes 2 and 3 read 8 B and write 8 B) as a fraction of the
    copy bandwidth measured in this process."""
    copy_gbps = cbg.hbm_copy_bandwidth(1 << 30, 10)
    its = []

    def on_iteration(it, chaos, nnz, ms_expand, ms_prune, ms_inflate):
        st = cbg.inflate_stats()
        passes = []
        for ms, per_entry in zip(st["ms"], (8.0, 16.0, 16.0)):
            gbps = per_entry * st["nnz"] / ms / 1e6 if ms > 0 else None
            passes.append(dict(ms=ms, gbps=gbps, fraction_of_copy=gbps / copy_gbps if gbps else None))
        its.append(dict(iteration=it, chaos=chaos, nnz=nnz, entries_inflated=st["nnz"], expand_ms=ms_expand,
                        prune_ms=ms_prune, inflate_ms=ms_inflate, inflate_passes=passes))

    t0 = time.perf_counter()
    labels, n = cbg.HipMCL(A, inflation=a.inflation, prunelimit=a.threshold, select=a.select, recover_num=a.recover,
                           recover_pct=a.pct, phases=a.phases, max_iterations=a.max_iterations,
                           on_iteration=on_iteration)
    wall = (time.perf_counter() - t0) * 1e3
    out = dict(scale=a.scale, ef=a.ef, inflation=a.inflation,
               params=dict(hardThreshold=a.threshold, selectNum=a.select, recoverNum=a.recover, recoverPct=a.pct),
               iterations=n, clusters=int(labels.max()) + 1 if len(labels) else 0, wall_ms=wall,
               hbm_copy_gbps=copy_gbps, moment_bounds=cbg.mcl_moment_bounds(), totals=cbg.hipmcl_stats(),
               per_iteration=its)
    path = a.out or os.path.join(REPO, "profiles", "hipmcl_s%d.json" % a.scale)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterate", action="store_true", help="run the whole HipMCL loop (profiles/hipmcl_s<scale>.json)")
    ap.add_argument("--inflation", type=float, default=2.0)
    ap.add_argument("--max-iterations", type=int, default=0)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--ef", type=int, default=16)
    ap.add_argument("--phases", type=int, default=-1, help="-1: from the device's free memory")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--select", type=int, default=1100)
    ap.add_argument("--recover", type=int, default=1400)
    ap.add_argument("--pct", type=float, default=0.9)
    ap.add_argument("--threshold", type=float, default=1e-4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cbg = _load()
    cbg.lib().cbg_set_device(0)
    g = cbg.CommGrid(0, 1, transport="host", host_comm=_Self())
    A = cbg.SpParMat.rmat(g, a.scale, a.ef)
    cnt, tot = A.tile.col_stats(-1.0, 1)  # column sums (the statistics kernel itself)
    A.tile.dim_apply(cbg.Column, np.where(tot > 0, 1.0 / np.maximum(tot, 1e-300), 1.0), "multiplies")
    if a.iterate:
        return iterate(cbg, A, a)
    B = A.copy()
    params = (a.threshold, a.select, a.recover, a.pct)
    copy_gbps = cbg.hbm_copy_bandwidth(1 << 30, 10)
    run(cbg, A, B, a.phases, params, digest=False)  # warm-up
    runs = [run(cbg, A, B, a.phases, params, digest=False) for _ in range(a.reps)]
    med = sorted(runs, key=lambda r: r["wall_ms"])[len(runs) // 2]
    # the pruning alone, twice on one fixed (inexact) product
    C = cbg.MemEfficientSpGEMM(A, B, 1)
    fixed = []
    for _ in range(2):
        P = cbg.MCLPruneRecoverySelect(C, *params)
        d = P.tile.digest()
        fixed.append((d["nnz"], d["hs"], d["hv"]))
        P.tile.free()
    C.tile.free()
    # exact values: the whole pruned product is independent of the phases
    h = A.tile.to_host()
    cnt = np.diff(h["cp"])
    col = np.repeat(h["jc"].astype(np.int64), cnt)
    h["val"] = (1 + (7 * h["ir"].astype(np.int64) + 13 * col) % 8).astype(np.float64) / 16
    Ax = cbg.SpParMat(cbg.Tile.from_dict(h), g, A.gm, A.gn)
    Bx = Ax.copy()
    xparams = (1.0 / 64, a.select, a.recover, 64.0)
    exact = [run(cbg, Ax, Bx, ph, xparams) for ph in (1, a.phases, 4)]
    st = med["stats"]
    two_pass = st["cols_selected"] > 0 and a.recover > 0
    ms = st["ms"]
    stats_bytes = 8.0 * st["entries_in"] * (2 if two_pass else 1)
    compact_bytes = 20.0 * st["entries_in"] + 12.0 * st["entries_out"]
    mult_ms = sum(p["mult"] for p in med["pieces"])
    out = dict(
        scale=a.scale, ef=a.ef, params=dict(hardThreshold=a.threshold, selectNum=a.select, recoverNum=a.recover,
                                            recoverPct=a.pct),
        phases=med["plan"]["phases"], reps=a.reps, wall_ms_runs=[r["wall_ms"] for r in runs], wall_ms=med["wall_ms"],
        multiply_ms=mult_ms, prune_ms=dict(ms, total=sum(ms.values())),
        prune_over_multiply=sum(ms.values()) / mult_ms if mult_ms else None,
        entries_in=st["entries_in"], entries_out=st["entries_out"], cols_recovered=st["cols_recovered"],
        cols_selected=st["cols_selected"], cols_recovered_after=st["cols_recovered_after"], pieces=st["pieces"],
        kselect_columns=st["kselect"], kselect_bounds=cbg.mcl_kselect_bounds(),
        hbm_copy_gbps=copy_gbps,
        stats_gbps=stats_bytes / ms["stats"] / 1e6 if ms["stats"] else None,
        compact_gbps=compact_bytes / ms["compact"] / 1e6 if ms["compact"] else None,
        per_piece=med["pieces"],
        prune_repeatable=fixed[0] == fixed[1], prune_fixed_input_digest=fixed[0],
        exact_params=dict(hardThreshold=xparams[0], selectNum=xparams[1], recoverNum=xparams[2], recoverPct=xparams[3]),
        exact_digests=[dict(phases=r["plan"]["phases"], pieces=r["stats"]["pieces"],
                            cols_selected=r["stats"]["cols_selected"], **r["digest"]) for r in exact],
        digests_equal=all(r["digest"] == exact[0]["digest"] for r in exact))
    out["stats_fraction_of_copy"] = out["stats_gbps"] / copy_gbps if out["stats_gbps"] else None
    out["compact_fraction_of_copy"] = out["compact_gbps"] / copy_gbps if out["compact_gbps"] else None
    path = a.out or os.path.join(REPO, "profiles", "mcl_bench_s%d.json" % a.scale)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "per_piece"}))
    if not out["digests_equal"] or not out["prune_repeatable"]:
        sys.exit("digests differ: " + json.dumps([out["exact_digests"], fixed]))


if __name__ == "__main__":
    main()
