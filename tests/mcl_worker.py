"""Worker of the multi-rank pruning tests (launched by torch.distributed.run).

usage: mcl_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py)

Every rank also runs the same calls on a 1 x 1 grid of its own and compares its tile
of the distributed result with its block of the 1 x 1 result, structure exactly and
values by bits: cbg_grid_kselect, cbg_grid_mcl_prune (all parameter sets) and
MemEfficientSpGEMM_MCL (phases 1 and 3, both exec modes).  Prints MCLOK per rank.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_cbg  # noqa: E402
from helpers import assert_tiles_bits_equal  # noqa: E402
import mcl_ref  # noqa: E402

E2E = (0.0625, 20, 30, 4.0)


class _Self:
    def bcast(self, comm, arr, root):
        pass

    def allgather(self, comm, data):
        return data


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
    one = cbg.CommGrid(0, 1, transport="host", host_comm=_Self())

    def mine(full):
        """this rank's block of a global host matrix"""
        r0, r1 = cbg.block_range(full["m"], pr, grid.prow)
        c0, c1 = cbg.block_range(full["n"], pc, grid.pcol)
        return cbg.sub_tile(full, r0, r1, c0, c1)

    # ---- k-select and MCLPruneRecoverySelect of a distributed matrix
    t = mcl_ref.multirank_case()
    D = cbg.SpParMat.from_global(grid, t)
    W = cbg.SpParMat.from_global(one, t)
    c0, c1 = cbg.block_range(t["n"], pc, grid.pcol)
    for k in (1, 3, 5, 700, 5000, 10 ** 6):  # 700 / 5000: the union of the ranks' multisets leaves the wave class
        got = D.Kselect(np.arange(c1 - c0), k)
        want = W.Kselect(np.arange(c0, c1), k)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (rank, k, np.flatnonzero(got != want)[:8])
    for (h, S, R, q) in mcl_ref.PARAM_SETS:
        got = cbg.MCLPruneRecoverySelect(D, h, S, R, q)
        want = cbg.MCLPruneRecoverySelect(W, h, S, R, q).tile.to_host()
        assert_tiles_bits_equal(want, mcl_ref.mcl_prune_ref(t, h, S, R, q))
        assert got.tile.digest()["unsorted"] == 0
        assert_tiles_bits_equal(got.tile.to_host(), mine(want))
    # ---- the pruned phased product
    a = mcl_ref.dyadic_values(cbg.rmat_tile(10, 16).to_host())
    A, B = cbg.SpParMat.from_global(grid, a), cbg.SpParMat.from_global(grid, a)
    A1, B1 = cbg.SpParMat.from_global(one, a), cbg.SpParMat.from_global(one, a)
    want = cbg.MemEfficientSpGEMM_MCL(A1, B1, 1, *E2E).tile.to_host()
    assert len(want["ir"]) < cbg.MemEfficientSpGEMM(A1, B1, 1).tile.nnz
    for exec_mode in (cbg.EXEC_PANEL, cbg.EXEC_STAGED):
        for phases in (1, 3):
            got = cbg.MemEfficientSpGEMM_MCL(A, B, phases, *E2E, exec_mode=exec_mode)
            assert_tiles_bits_equal(got.tile.to_host(), mine(want))
    pieces = []
    cbg.MemEfficientSpGEMM_MCL(A, B, 3, *E2E, on_phase=lambda p, off, tile: pieces.append((off, tile.nnz)))
    assert sum(p[1] for p in pieces) == len(mine(want)["ir"]) and len(pieces) >= 3
    grid.destroy()
    hc.allgather(0, b"x")
    print("MCLOK", flush=True)


if __name__ == "__main__":
    main()
