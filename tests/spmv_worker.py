"""Worker of the multi-rank SpMV tests (launched by torch.distributed.run), and the loaders of the
spmv fixtures the single-process tests share.

usage: spmv_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py)

Every rank runs cbg.SpMV and cbg.SpMV_sparse under both semirings on the `rmat` and `rect` fixtures
(tests/golden/spmv_*.npz) and on the `split` case, whose rows have (16, 17), (4096, 4097), (0, 30) and
(30, 0) entries left and right of the column cut.  The results have to be spmv_ref's bits with the
grid's column cut, identical on all ranks (the bits are allgathered); on `dyadic` they are the
reference's own 1-rank bits.  Over the host transport the dense product also runs on full 3 x 3 and 5 x 5
matrices (blocks of 1 and 2, the last one longer) and on a row whose sum depends on the fold order.  A tile handed to a grid of another shape is refused with DIMMISMATCH
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


def tiny_case(gn):
    """a full gn x gn matrix and x of dyadic values (every sum exact): on two ranks a side the blocks are
    gn // 2 long and the last one longer, none empty"""
    key = ("tiny", gn)
    if key not in _cache:
        rng = np.random.default_rng(gn)
        row, col = np.divmod(np.arange(gn * gn), gn)
        val = rng.integers(1, 64, gn * gn) / 8.0 * rng.choice([-1.0, 1.0], gn * gn)
        _cache[key] = hr.from_coo(gn, gn, row, col, val), rng.integers(-32, 33, gn) / 4.0
    return _cache[key]


def cancel_case():
    """row 0 holds 1e16 left of the column cut n // 2 and -1e16, 1.0 right of it: its PlusTimes sum depends
    on the order (one rank: (1e16 - 1e16) + 1.0), and the grid's is the ranks' partial sums folded in rank order"""
    if "cancel" not in _cache:
        t = hr.from_coo(2, 4, [0, 0, 0, 1], [0, 2, 3, 1], [1e16, -1e16, 1.0, 3.0])
        _cache["cancel"] = t, np.ones(4)
    return _cache["cancel"]


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
    if mode == "gpu":
        for gn in (3, 5):  # uneven blocks through the gather of the row blocks
            tt, tx = tiny_case(gn)
            for s, sr in SEMIRINGS:
                check("tiny%d" % gn, s, sr, tt, tx, {})
        tc, cx = cancel_case()
        check("cancel", "pt", sv.PLUS_TIMES, tc, cx, {})
        # 1e16 + (-1e16 + 1.0): the 1.0 is lost in the right rank's partial sum, and kept without the cut
        assert sv.spmv(tc, cx, sv.PLUS_TIMES, [2])[0] == 0.0 and sv.spmv(tc, cx, sv.PLUS_TIMES)[0] == 1.0
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
