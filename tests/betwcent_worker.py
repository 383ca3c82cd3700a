"""Worker of the multi-rank BetwCent tests (launched by torch.distributed.run).

usage: betwcent_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py)

Every rank runs BetwCent on every fixture (tests/golden/betwcent_*.npz) with the fixture's
roots, in two batch sizes (the last batch shorter): bc has to be within the fixture's bound
of the exact values, and identical on all ranks (its bits are allgathered).  On a square grid AT
is left to the library (the transpose); elsewhere it is handed over, and leaving it out has to
give NOTSQUARE on every rank.  A batch with fewer roots than the grid has columns (one root, or a last batch
of one) is refused with INVALIDPARAMS on every rank of 1 x 2 and 2 x 2, and computed within the bound on 2 x 1.  The level sizes every rank's callback sees are those of the exact
restatement.  Prints BETWCENTOK per rank.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_cbg  # noqa: E402
import betwcent_ref as br  # noqa: E402
import hipmcl_ref as hr  # noqa: E402

CASES = ("lattice", "rmat", "components")


def load_case(name):
    z = np.load(os.path.join(HERE, "golden", f"betwcent_{name}.npz"))
    n = int(z["n"])
    A = hr.from_coo(n, n, z["row"], z["col"], np.ones(len(z["row"])))
    AT = hr.from_coo(n, n, z["col"], z["row"], np.ones(len(z["row"])))
    return z, A, AT


def bound(z, nroots, batches):
    K = br.bound_factor(int(z["depth"]), int(z["degree"]), nroots, batches)
    return K * 2.0 ** -52 * (z["bc_exact"] + nroots)


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

    for name in (CASES if mode != "rccl" else ("rmat",)):  # RCCL: one fixture, the transport is what differs
        z, a, at = load_case(name)
        roots = z["roots"]
        A = cbg.SpParMat.from_global(grid, a)
        AT = cbg.SpParMat.from_global(grid, at) if pr != pc else None
        for batch in ((4, 6) if len(roots) == 8 else (6, 9)):  # no batch narrower than the grid
            seen = []
            bc = cbg.BetwCent(A, roots, batch, AT=AT, on_level=lambda b, lv, nnz: seen.append((b, lv, nnz)))
            nb = -(-len(roots) // batch)
            err = np.abs(bc - z["bc_exact"])
            assert np.all(err <= bound(z, len(roots), nb)), (rank, name, batch, float(err.max()))
            want = br.brandes(a, roots.tolist(), batch)["levels"]
            assert seen == [(b, k + 1, s) for b, lv in enumerate(want) for k, s in enumerate(lv)], (rank, name, batch)
            mine = bc.view(np.uint64).tobytes()
            everyone = hc.allgather(0, mine)
            assert everyone == mine * world, (rank, name, batch)
            st = cbg.betwcent_stats()
            assert st["batches"] == nb and st["levels"] == len(seen) and st["fringe_entries"] == sum(s[2] for s in seen)
        for narrow in ((roots[:1], 4), (roots[:5], 4), (roots, len(roots) - 1)):  # a last batch of one root
            if pc > 1:  # fewer roots than grid columns: refused on every rank before any device work
                try:
                    cbg.BetwCent(A, narrow[0], narrow[1], AT=AT)
                    raise AssertionError("a batch narrower than the %d x %d grid was taken" % (pr, pc))
                except cbg.CbgError as e:
                    assert e.code == cbg.INVALIDPARAMS and "fewer roots" in str(e), e
            elif name == "rmat":  # a grid of one column takes any batch
                bc = cbg.BetwCent(A, narrow[0], narrow[1], AT=AT)
                ex = np.array([float(x) for x in br.brandes(a, narrow[0].tolist())["bc"]])
                nr = len(narrow[0])
                K = br.bound_factor(int(z["depth"]), int(z["degree"]), nr, -(-nr // narrow[1]))
                assert np.all(np.abs(bc - ex) <= K * 2.0 ** -52 * (ex + nr)), (rank, name, narrow[1])
        if pr != pc:  # without AT the transpose needs a square grid: the same code on every rank
            try:
                cbg.BetwCent(A, roots, 4)
                raise AssertionError("no error without AT on a %d x %d grid" % (pr, pc))
            except cbg.CbgError as e:
                assert e.code == cbg.NOTSQUARE, e
    grid.destroy()
    hc.allgather(0, b"x")
    print("BETWCENTOK", flush=True)


if __name__ == "__main__":
    main()
