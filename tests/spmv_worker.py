"""Worker of the multi-rank SpMV tests (launched by torch.distributed.run), and the loaders of the
spmv fixtures the single-process tests share.

usage: spmv_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py)

Every rank runs cbg.SpMV and cbg.SpMV_sparse under both semirings on the `rmat` and `rect` fixtures
(tests/golden/spmv_*.npz) and on the `split` case, whose rows have (16, 17), (4096, 4097), (0, 30) and
(30, 0) entries left and right of the column cut.  The results have to be spmv_ref's bits with the
grid's column cut, identical on all ranks (the bits are allgathered); on `dyadic` they are the
reference's own 1-rank bits.  A tile handed to a grid of another shape is refused with DIMMISMATCH
on every rank.  Prints SPMVOK per rank.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_cbg  # noqa: E402
import colsum_ref as cr  # noqa: E402
import hipmcl_ref as hr  # noqa: E402
import spmv_ref as sv  # noqa: E402

CASES = ("rmat", "dyadic", "rect")
SEMIRINGS = (("pt", sv.PLUS_TIMES), ("mp", sv.MIN_PLUS))
SPARSE = ("even", "k16")
_cache = {}


def load_case(name):
    """-> (z, {s: DCSC dict}) of tests/golden/spmv_<name>.npz.  Cached: do not modify"""
    if name not in _cache:
        z = np.load(os.path.join(HERE, "golden", f"spmv_{name}.npz"))
        m, n = int(z["m"]), int(z["n"])
        _cache[name] = z, {s: hr.from_coo(m, n, z["row"], z["col"], z["val_" + s]) for s, _ in SEMIRINGS}
    return _cache[name]


# (entries left, entries right) of the column cut n // 2
SPLIT_ROWS = ((16, 17), (4096, 4097), (0, 30), (30, 0))


def split_case(n=8400):
    """2 rows per entry of SPLIT_ROWS and an empty row after each pair, `wide` values, x U[-1, 1)"""
    if "split" not in _cache:
        rng = np.random.default_rng(4243)
        half = n // 2
        rows, cols, r = [], [], 0
        for a, b in SPLIT_ROWS:
            for _ in range(2):
                c = np.concatenate([np.sort(rng.choice(half, a, replace=False)),
                                    half + np.sort(rng.choice(n - half, b, replace=False))])
                rows.append(np.full(len(c), r))
                cols.append(c)
                r += 1
            r += 1
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        val = cr.pattern_values(rng, "wide", len(rows))
        _cache["split"] = hr.from_coo(r + 1, n, rows, cols, val), rng.uniform(-1.0, 1.0, n)
    return _cache["split"]


def main():
    mode, pr, pc = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    cbg = load_cbg()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == pr * pc
    port = int(os.environ["MASTER_PORT"]) + 1
    if mode == "rccl":
        os.environ["NCCL_HOSTID"] = "cbg-test-rank-%d" % rank
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_IB_DISABLE", "1")
    cbg.lib()
    hc = cbg.TcpHostComm(rank, world, pr, pc, "127.0.0.1", port)
    if mode == "rccl":
        uid = hc.bcast_object(cbg.CommGrid.unique_id() if rank == 0 else None, root=0)
        grid = cbg.CommGrid(rank, world, pr, pc, unique_id=uid, transport="rccl")
        if rank == 0:
            print("transport rccl, %d ranks" % world, flush=True)
    else:
        grid = cbg.CommGrid(rank, world, pr, pc, transport="host", host_comm=hc)

    def check(name, s, sr, t, x, sparse, ref_dense=None, ref_sparse=None):
        cuts = [(t["n"] // pc) * q for q in range(1, pc)]
        A = cbg.SpParMat.from_global(grid, t)
        before = A.tile.digest()
        At = A.tile.transpose() if (pr, pc) == (2, 2) else None
        y = cbg.SpMV(A, x, sr, At=At)
        want = sv.spmv(t, x, sr, cuts)
        assert np.array_equal(sv.bits(y), sv.bits(want)), (rank, name, s, "dense")
        if ref_dense is not None:
            assert np.array_equal(sv.bits(y), sv.bits(ref_dense)), (rank, name, s, "dense vs 1 x 1")
        mine = y.tobytes()
        for k, ids in sparse.items():
            yi, yv = cbg.SpMV_sparse(A, ids, x[ids], sr)
            wi, wv = sv.spmspv(t, ids, x[ids], sr, cuts)
            assert np.array_equal(yi, wi) and np.array_equal(sv.bits(yv), sv.bits(wv)), (rank, name, s, k)
            if ref_sparse is not None:
                assert np.array_equal(yi, ref_sparse[k][0]) and np.array_equal(sv.bits(yv), sv.bits(ref_sparse[k][1]))
            mine += yi.tobytes() + yv.tobytes()
        assert hc.allgather(0, mine) == mine * world, (rank, name, s)
        after = A.tile.digest()
        assert (after["hs"], after["hv"]) == (before["hs"], before["hv"])
        return A

    for name in CASES:
        z, ts = load_case(name)
        for s, sr in SEMIRINGS:
            sparse = {k: z["xs_" + k] for k in SPARSE}
            exact = name == "dyadic"
            A = check(name, s, sr, ts[s], z["x_" + s], sparse, z["y_" + s] if exact else None,
                      {k: (z[f"ys_{s}_{k}_ind"], z[f"ys_{s}_{k}_val"]) for k in SPARSE} if exact else None)
    t, x = split_case()
    for s, sr in SEMIRINGS:
        A = check("split", s, sr, t, x, dict(all=np.arange(t["n"]), even=np.arange(0, t["n"], 2)))
    if world > 1:  # the tile is not the block of a matrix one row and one column longer
        try:
            cbg.SpMV(cbg.SpParMat(A.tile, grid, t["m"] + pr, t["n"] + pc), np.zeros(t["n"] + pc))
            raise AssertionError("a misplaced tile was taken")
        except cbg.CbgError as e:
            assert e.code == cbg.DIMMISMATCH, e
    grid.destroy()
    hc.allgather(0, b"x")
    print("SPMVOK", flush=True)


if __name__ == "__main__":
    main()
