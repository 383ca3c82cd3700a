"""Worker of the multi-rank sparse-indexing tests (launched by torch.distributed.run).

usage: spref_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py)

Every rank runs the same calls on a 1 x 1 grid of its own and compares its tile of the
distributed result, by bits, with its block of the 1 x 1 result: the permutation, the
repeats and the rectangular indexings of the 301 x 257 matrix (no extent divisible by 2),
an increasing selection (no sort), "all" on either side, nri = 1 (a grid row with no rows)
and a block-diagonal input whose off-diagonal tiles are empty.  HipMCL with RemoveIsolated
and RandPermute on both golden cases gives the 1 x 1 labels, iteration count and working
numbering.  LoadImbalance of a matrix with every entry in its top-left quarter is the rank
count, and after RandPermute(seed 1) the value of spref_ref.load_imbalance on this grid,
without a tolerance.  Prints SPREFOK per rank.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_cbg  # noqa: E402
from helpers import assert_tiles_bits_equal  # noqa: E402
import hipmcl_ref as hr  # noqa: E402
import spref_ref as sr  # noqa: E402


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

    def check(t, ri, ci, what):
        D, W = cbg.SpParMat.from_global(grid, t), cbg.SpParMat.from_global(one, t)
        got = D.SubsRef(ri, ci)
        st = cbg.spref_stats()  # the distributed call's
        want = W.SubsRef(ri, ci).tile.to_host()
        assert_tiles_bits_equal(want, sr.spref(t, ri, ci))
        assert got.tile.digest()["unsorted"] == 0, (rank, what)
        assert (got.gm, got.gn) == (want["m"], want["n"]), (rank, what)
        assert_tiles_bits_equal(got.tile.to_host(), mine(want))
        assert_tiles_bits_equal(D.tile.to_host(), mine(t))  # the input is left as it was
        return st

    t = sr.main_tile()
    cases = sr.index_cases(t["m"], t["n"])
    for name in ("perm", "repeats", "repeats_tall", "rect", "increasing", "rows_all", "cols_all", "no_rows"):
        st = check(t, *cases[name], name)
        if name == "increasing":
            assert st["sorted_wave"] + st["sorted_lds"] + st["sorted_radix"] == 0, (rank, st)
        if name == "perm" and world > 1:
            assert st["bytes_recv"] > 0, (rank, st)
    check(t, np.array([19]), cases["perm"][1], "nri = 1")
    check(t, cases["perm"][0], np.array([19]), "nci = 1")
    # a block-diagonal matrix leaves the off-diagonal tiles of a 2 x 2 grid empty
    bd = hr.planted()
    half = bd["n"] // 2
    r, c = bd["ir"].astype(np.int64), hr.cols_of(bd)
    same = (r < half) == (c < half)
    bd = hr.from_coo(bd["n"], bd["n"], r[same], c[same], bd["val"][same])
    if pr == 2 and pc == 2:
        assert (mine(bd)["cp"][-1] == 0) == (grid.prow != grid.pcol)
    p = sr.rand_perm(bd["n"], 5)
    check(bd, p, p, "block diagonal")
    # an index outside the matrix: the same code on every rank, and the grid still works
    D = cbg.SpParMat.from_global(grid, t)
    try:
        D.SubsRef([t["m"]], None)
        raise AssertionError("an index equal to the extent was accepted")
    except cbg.CbgError as e:
        assert e.code == cbg.INVALIDPARAMS
    check(t, *cases["rect"], "after the error")

    # ---- HipMCL with both steps
    for base in (hr.planted(), hr.hub()):
        g = sr.pad_isolated(base, sr.pad_positions(base["n"]))
        for ps in hr.PARAM_SETS:
            infl, h, S, R, q = ps
            kw = dict(inflation=infl, prunelimit=h, select=S, recover_num=R, recover_pct=q, remove_isolated=True,
                      randpermute=True, perm_seed=1, return_work_ids=True)
            labels, its, work = cbg.HipMCL(cbg.SpParMat.from_global(grid, g), **kw)
            wl, wi, ww = cbg.HipMCL(cbg.SpParMat.from_global(one, g), **kw)
            assert its == wi and np.array_equal(labels, wl) and np.array_equal(work, ww), (rank, its, wi)
        D = cbg.SpParMat.from_global(grid, g)
        B, ids = cbg.RemoveIsolated(D)
        assert np.array_equal(ids, sr.nonisolated(g))
        assert_tiles_bits_equal(B.tile.to_host(), mine(sr.spref(g, ids, ids)))

    # ---- LoadImbalance: every entry in the top-left quarter
    rng = np.random.default_rng(6)
    n = 120
    key = np.unique(rng.integers(0, n // 2, 900) * n + rng.integers(0, n // 2, 900))
    q = hr.from_coo(n, n, key // n, key % n, np.ones(len(key)))
    D = cbg.SpParMat.from_global(grid, q)
    assert D.LoadImbalance() == sr.load_imbalance(q, pr, pc) == float(world), (rank, D.LoadImbalance())
    P, p = cbg.RandPermute(D, 1)
    assert np.array_equal(p, sr.rand_perm(n, 1))
    assert P.LoadImbalance() == sr.load_imbalance(sr.spref(q, p, p), pr, pc), (rank, P.LoadImbalance())
    if world > 1:
        assert P.LoadImbalance() < D.LoadImbalance()
    grid.destroy()
    hc.allgather(0, b"x")
    print("SPREFOK", flush=True)


if __name__ == "__main__":
    main()
