"""Worker of the multi-rank BFS tests (launched by torch.distributed.run).

usage: bfs_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py); coretail only

Every rank runs cbg.BFS on every fixture (tests/golden/bfs_*.npz) and root under AUTO, and on the
first root in one forced direction (top-down on grids of one row, bottom-up elsewhere; the local
transpose handed over on 2 x 2).  parents have to be the fixture's bits and levels the
restatement's, identical on all ranks (the bits are allgathered); the steps every rank's callback
sees and the grid-independent stats are the restatement's.  A root outside the matrix is refused
with INVALIDPARAMS on every rank.  Over the host transport every root of a path of 3 and of 5 vertices
(row blocks of 1 | 2 and 2 | 3) has to give valid parents and the restatement's levels.  Prints BFSOK per rank.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_cbg  # noqa: E402
import bfs_ref  # noqa: E402
import hipmcl_ref as hr  # noqa: E402

CASES = ("rmat", "coretail", "directed", "path")
GRID_FREE = ("levels", "reached", "edges", "push_steps", "pull_steps")  # stats that no grid shape changes


def load_case(name):
    z = np.load(os.path.join(HERE, "golden", f"bfs_{name}.npz"))
    n = int(z["n"])
    return z, hr.from_coo(n, n, z["row"], z["col"], np.ones(len(z["row"])))


def tiny_case(gn):
    """the undirected path 0 - 1 - ... - gn - 1: every vertex is reached from every root, the last
    (longer) block included"""
    v = np.arange(gn - 1)
    return hr.from_coo(gn, gn, np.concatenate([v, v + 1]), np.concatenate([v + 1, v]), np.ones(2 * (gn - 1)))


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

    forced = "topdown" if pr == 1 else "bottomup"
    for name in (CASES if mode != "rccl" else ("coretail",)):
        z, a = load_case(name)
        A = cbg.SpParMat.from_global(grid, a)
        before = A.tile.digest()
        At = A.tile.transpose() if (pr, pc) == (2, 2) else None
        for k, root in enumerate(z["roots"].tolist()):
            for direction in (("auto", forced) if k == 0 else ("auto",)):
                want = bfs_ref.bfs(a, root, direction)
                seen = []
                parents, levels = cbg.BFS(A, root, direction, on_level=lambda *s: seen.append(s), At=At)
                assert np.array_equal(parents, z["parents"][k]), (rank, name, root, direction)
                assert np.array_equal(levels, want["levels"]) and np.array_equal(levels, z["levels"][k]), (rank, name, root)
                assert seen == want["steps"], (rank, name, root, direction, seen[:6], want["steps"][:6])
                st = cbg.bfs_stats()
                assert {s: st[s] for s in GRID_FREE} == {s: want["stats"][s] for s in GRID_FREE}, (rank, name, root, st)
                mine = parents.tobytes() + levels.tobytes()
                assert hc.allgather(0, mine) == mine * world, (rank, name, root, direction)
        after = A.tile.digest()
        assert (after["hs"], after["hv"]) == (before["hs"], before["hv"])
        for bad in (-1, a["n"]):
            try:
                cbg.BFS(A, bad)
                raise AssertionError("root %d was taken" % bad)
            except cbg.CbgError as e:
                assert e.code == cbg.INVALIDPARAMS, e
    if mode == "gpu":
        for gn in (3, 5):  # uneven blocks through the gather of the row blocks: 1 | 2 and 2 | 3 vertices
            a = tiny_case(gn)
            A = cbg.SpParMat.from_global(grid, a)
            for root in range(gn):
                want = bfs_ref.bfs(a, root)
                parents, levels = cbg.BFS(A, root)
                assert bfs_ref.validate(a, root, parents, levels) is None, (rank, gn, root, parents, levels)
                assert np.array_equal(levels, want["levels"]), (rank, gn, root, levels)
                mine = parents.tobytes() + levels.tobytes()
                assert hc.allgather(0, mine) == mine * world, (rank, gn, root)
    grid.destroy()
    hc.allgather(0, b"x")
    print("BFSOK", flush=True)


if __name__ == "__main__":
    main()
