#!/usr/bin/env python3
"""y = A x (cbg_tile_spmv, cbg_tile_spmspv) on one GPU.

R-MAT (default scale 18, edge factor 16) with U[-1, 1) values, its transpose built once, x and y resident
on the device.  Writes one JSON line to --out (default profiles/spmv_s<scale>.json) and prints it.

  dense   per semiring: `reps` products on one stream between two device events, after a warm-up; reps is
          chosen so that the window lasts about --seconds.  ms per product, G nnz/s, the algorithmic bytes
          (12 B per stored entry: row id and value of the transpose; 8 B of x per stored column; 8 B of y
          per row) over that time in GB/s, and its ratio to cbg_hbm_copy_bandwidth measured in this
          process.  ms_kernels is the span between the library's own two events around one product's
          kernels (cbg_last_spmv_stats): the difference to ms is what the host adds between products.
  sparse  x with nx = n / 1024 ... n random columns (host vectors in and out, as the entry point takes
          them): the median over --sparse-reps calls of the library's event span (expansion, sort,
          reduction and the two readbacks in between) and of the host clock around the call.
          crossover_nx: the smallest nx of the sweep whose event span exceeds ms_kernels of the dense
          PlusTimes product (null: none does).
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from __graft_entry__ import _load  # noqa: E402


class Hip:
    """the few runtime calls the timing needs (the library's own copy of the runtime)"""

    def __init__(self):
        self.l = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(f"hip error {rc}")

    def stream(self):
        s = ctypes.c_void_p()
        self.ok(self.l.hipStreamCreate(ctypes.byref(s)))
        return s

    def event(self):
        e = ctypes.c_void_p()
        self.ok(self.l.hipEventCreate(ctypes.byref(e)))
        return e

    def record(self, e, s):
        self.ok(self.l.hipEventRecord(e, s))

    def elapsed_ms(self, e0, e1):
        self.ok(self.l.hipEventSynchronize(e1))
        ms = ctypes.c_float()
        self.ok(self.l.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        return float(ms.value)


def device_vector(cbg, v):
    """len(v) doubles on the device: the values of a one-column tile"""
    n = len(v)
    return cbg.Tile.from_host(n, 1, [0, n], [0], np.arange(n), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=18)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--sparse-reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=1810)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cbg = _load()
    L = cbg.lib()
    L.cbg_set_device(0)
    hip = Hip()
    A = cbg.rmat_tile(a.scale, a.edgefactor)
    A.set_random_values()
    At = A.transpose()  # once for all the products
    m, n, nnz, nzc = A.m, A.n, A.nnz, A.nzc
    rng = np.random.default_rng(a.seed)
    x = rng.uniform(-1.0, 1.0, n)
    dx, dy = device_vector(cbg, x), device_vector(cbg, np.zeros(m))
    copy_gbps = cbg.hbm_copy_bandwidth(1 << 30, 10)
    bytes_alg = 12 * nnz + 8 * nzc + 8 * m
    s, e0, e1 = hip.stream(), hip.event(), hip.event()

    def product(sr):
        rc = L.cbg_tile_spmv(None, ctypes.byref(At.c), sr, dx.c.val, dy.c.val, 1, s)
        if rc:
            raise RuntimeError(L.cbg_last_error().decode())

    def window(sr, reps):
        hip.record(e0, s)
        for _ in range(reps):
            product(sr)
        hip.record(e1, s)
        return hip.elapsed_ms(e0, e1)

    res = dict(scale=a.scale, edgefactor=a.edgefactor, m=m, n=n, nnz=nnz, stored_columns=nzc, bounds=cbg.spmv_bounds(),
               copy_gbps=copy_gbps, algorithmic_bytes=bytes_alg, dense={}, sparse=[])
    for name, sr in (("plus_times", cbg.PLUS_TIMES), ("min_plus", cbg.MIN_PLUS)):
        window(sr, a.warmup)  # code objects, the pool's blocks
        per = window(sr, 200) / 200
        reps = int(min(max(math.ceil(a.seconds * 1e3 / per), 200), 200000))
        ms = window(sr, reps) / reps
        st = cbg.spmv_stats()  # the last product's
        y = dy.to_host()["val"].copy()
        host = A.spmv(x, sr, At=At)
        assert np.array_equal(y.view(np.uint64), host.view(np.uint64)), "device-pointer and host call disagree"
        gbps = bytes_alg / (ms * 1e-3) / 1e9
        res["dense"][name] = dict(reps=reps, ms=ms, ms_kernels=st["ms"], gnnz_per_s=nnz / (ms * 1e-3) / 1e9, gbps=gbps,
                                  fraction_of_copy=gbps / copy_gbps,
                                  gbps_kernels=bytes_alg / (st["ms"] * 1e-3) / 1e9,
                                  fraction_of_copy_kernels=bytes_alg / (st["ms"] * 1e-3) / 1e9 / copy_gbps,
                                  rows_group=st["rows_group"], rows_wave=st["rows_wave"], rows_long=st["rows_long"],
                                  chunks=st["chunks"])
    dense_ms = res["dense"]["plus_times"]["ms_kernels"]
    crossover = None
    nx = max(n // 1024, 1)
    while True:
        ids = np.sort(rng.choice(n, nx, replace=False)) if nx < n else np.arange(n)
        A.spmspv(ids, x[ids])  # warm-up
        ev, host, st = [], [], None
        for _ in range(a.sparse_reps):
            cbg.synchronize()
            t0 = time.perf_counter()
            yi, yv = A.spmspv(ids, x[ids])
            host.append((time.perf_counter() - t0) * 1e3)
            st = cbg.spmv_stats()
            ev.append(st["ms"])
        row = dict(nx=int(nx), products=st["products"], units=st["units"], entries_out=st["entries_out"],
                   ms_events=float(np.median(ev)), ms_host=float(np.median(host)))
        res["sparse"].append(row)
        if crossover is None and row["ms_events"] > dense_ms:
            crossover = int(nx)
        if nx >= n:
            break
        nx = min(nx * 4, n)
    res["crossover_nx"] = crossover
    line = json.dumps(res)
    out = a.out or os.path.join(REPO, "profiles", f"spmv_s{a.scale}.json")
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
