"""Worker of the multi-rank HipMCL tests (launched by torch.distributed.run).

usage: hipmcl_worker.py <mode> <grid_rows> <grid_cols>
  mode "gpu":  the grid's collectives over the host (TCP) transport, the ranks sharing one GPU
  mode "rccl": over RCCL (one NCCL_HOSTID per rank: its socket transport, see mp_worker.py)

Every rank also runs the same calls on a 1 x 1 grid of its own and compares its tile
of the distributed result with its block of the 1 x 1 result, structure exactly and
values by bits: the four column reductions, MakeColStochastic and Chaos on
mcl_ref.multirank_case (dyadic values: every sum is exact, so the ranks' split of a
column does not show), the loops and the connected components on square matrices.
The fused Inflate is compared by bits with the four-call composition on the same
grid; against the 1 x 1 result it can differ in the last bits (the normalised values
are not dyadic and a column's sum is split between the ranks), so that comparison
allows the sums' rounding -- except on grids of one row (1 x 2), where no column is
split and the bits must be equal.  On inexact values (colsum_ref.split_case: per-rank lengths
at the class bounds of the column sums, columns empty in one row block) the four reductions,
MakeColStochastic, Chaos and Inflate(2.0) have the bits of the order-exact restatement summed
row block by row block and combined in rank order (tests/colsum_ref.py) -- on two row blocks
not the bits of the 1 x 1 run, which the restatement itself shows.  The phased SUMMA on a block-diagonal matrix (empty
off-diagonal tiles on 2 x 2) equals the 1 x 1 product by bits.  HipMCL on both golden
cases: the 1 x 1 partition and iteration count.  Prints HIPMCLOK per rank.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from conftest import load_cbg  # noqa: E402
from helpers import assert_tiles_bits_equal  # noqa: E402
import colsum_ref as cr  # noqa: E402
import hipmcl_ref as hr  # noqa: E402
import mcl_ref  # noqa: E402


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

    def bits(x):
        return np.ascontiguousarray(x, np.float64).view(np.uint64)

    # ---- column reductions, MakeColStochastic, Chaos, Inflate
    t = mcl_ref.multirank_case()
    t = dict(t, val=np.round(t["val"] * 1024) / 1024)  # every value a multiple of 2^-10: exact sums
    keep = t["val"] > 0
    tp = hr.from_coo(t["m"], t["n"], t["ir"][keep], hr.cols_of(t)[keep], t["val"][keep])
    c0, c1 = cbg.block_range(t["n"], pc, grid.pcol)
    for src in (t, tp, mcl_ref.dyadic_values(t)):
        D, W = cbg.SpParMat.from_global(grid, src), cbg.SpParMat.from_global(one, src)
        for what, ident in (("sum", 0.0), ("max", 0.0), ("max", -1e300), ("sumsq", 0.0), ("count", 0.0), ("sum", -3.0)):
            got, want = D.Reduce(cbg.Column, what, ident), W.Reduce(cbg.Column, what, ident)
            assert np.array_equal(bits(want), bits(hr.reduce_cols(src, what, ident))), (rank, what)
            assert np.array_equal(bits(got), bits(want[c0:c1])), (rank, what, ident)
        assert D.Chaos() == W.Chaos() == hr.chaos(src)
    D, W = cbg.SpParMat.from_global(grid, tp), cbg.SpParMat.from_global(one, tp)
    D.MakeColStochastic()
    W.MakeColStochastic()
    want = W.tile.to_host()
    assert_tiles_bits_equal(want, hr.make_col_stochastic(tp))
    assert_tiles_bits_equal(D.tile.to_host(), mine(want))
    for power in (2.0, 1.7):
        F, C, W = (cbg.SpParMat.from_global(g, tp) for g in (grid, grid, one))
        cf = F.Inflate(power)
        C.MakeColStochastic()
        cc = C.Chaos()
        C.Apply("pow", power)
        C.MakeColStochastic()
        assert bits([cf])[0] == bits([cc])[0], (rank, cf, cc)
        assert_tiles_bits_equal(F.tile.to_host(), C.tile.to_host())
        cw = W.Inflate(power)
        got, want = F.tile.to_host(), mine(W.tile.to_host())
        assert np.array_equal(got["ir"], want["ir"]) and np.array_equal(got["cp"], want["cp"])
        if pr == 1:  # every column lives on one rank: nothing is split, the bits are the 1 x 1 run's
            assert_tiles_bits_equal(got, want)
            assert bits([cf])[0] == bits([cw])[0], (rank, cf, cw)
            continue
        # a column of n entries: its sum's rounding is at most n eps relative, twice (two sums)
        lens = np.repeat(hr.reduce_cols(tp, "count")[c0:c1][got["jc"]], np.diff(got["cp"]))
        assert np.all(np.abs(got["val"] - want["val"]) <= 4 * lens * np.finfo(np.float64).eps * want["val"])
        assert abs(cf - cw) <= 4 * 30000 * np.finfo(np.float64).eps * max(cw, 1.0)

    # ---- inexact values: the bits of the order-exact restatement, row block by row block
    for pattern in ("uniform", "normal"):
        x = cr.split_case(pattern)
        cuts = [cbg.block_range(x["m"], pr, i)[0] for i in range(1, pr)]
        assert (cuts == [x["m"] // 2]) if pr == 2 else not cuts
        c0, c1 = cbg.block_range(x["n"], pc, grid.pcol)
        D = cbg.SpParMat.from_global(grid, x)
        for what, ident in (("sum", 0.0), ("sum", -3.0), ("sumsq", 0.0), ("max", 0.0), ("max", -1e300), ("count", 0.0)):
            got, want = D.Reduce(cbg.Column, what, ident), cr.reduce_cols_ordered(x, what, ident, cuts)
            assert np.array_equal(bits(got), bits(want[c0:c1])), (rank, pattern, what, ident)
            if pr == 2 and what in ("sum", "sumsq"):  # not the 1 x 1 run's bits: the split shows
                assert not np.array_equal(bits(want), bits(cr.reduce_cols_ordered(x, what, ident)))
        assert bits([D.Chaos()])[0] == bits([cr.chaos_ordered(x, cuts)])[0], (rank, pattern)
        if pattern != "uniform":
            continue
        D.MakeColStochastic()
        want = cr.make_col_stochastic_ordered(x, cuts)
        assert_tiles_bits_equal(D.tile.to_host(), mine(want))
        F = cbg.SpParMat.from_global(grid, x)
        cf = F.Inflate(2.0)
        want, wc = cr.inflate_ordered(x, 2.0, cuts=cuts)
        assert bits([cf])[0] == bits([wc])[0], (rank, cf, wc)
        assert_tiles_bits_equal(F.tile.to_host(), mine(want))
        if pr == 2:
            whole, _ = cr.inflate_ordered(x, 2.0)
            assert not np.array_equal(bits(want["val"]), bits(whole["val"]))

    # ---- loops and connected components (square matrices)
    for sq in (hr.loops_case(), hr.loops_case(seed=8, n=41), hr.planted()):
        n = sq["n"]
        lv = (np.arange(n) + 1) / 64.0
        D, W = cbg.SpParMat.from_global(grid, sq), cbg.SpParMat.from_global(one, sq)
        assert np.array_equal(cbg.Interpret(D), hr.interpret(sq))
        assert D.RemoveLoops() == W.RemoveLoops() == hr.remove_loops(sq)[1]
        assert D.tile.digest()["unsorted"] == 0
        assert_tiles_bits_equal(D.tile.to_host(), mine(W.tile.to_host()))
        for replace in (False, True):
            for src in (sq, hr.remove_loops(sq)[0]):
                D, W = cbg.SpParMat.from_global(grid, src), cbg.SpParMat.from_global(one, src)
                D.AddLoops(lv, replace)
                W.AddLoops(lv, replace)
                want = W.tile.to_host()
                assert_tiles_bits_equal(want, hr.add_loops(src, lv, replace))
                assert D.tile.digest()["unsorted"] == 0
                assert_tiles_bits_equal(D.tile.to_host(), mine(want))
        D, W = cbg.SpParMat.from_global(grid, sq), cbg.SpParMat.from_global(one, sq)
        D.AdjustLoops()
        W.AdjustLoops()
        want = W.tile.to_host()
        assert_tiles_bits_equal(want, hr.adjust_loops(sq))
        assert_tiles_bits_equal(D.tile.to_host(), mine(want))
    rng = np.random.default_rng(5)
    perm = rng.permutation(1500)
    path = hr.from_coo(1500, 1500, perm[:-1], perm[1:], np.ones(1499))
    assert cbg.Interpret(cbg.SpParMat.from_global(grid, path)).max() == 0
    e = rng.integers(0, 1500, (2, 700))
    key = np.unique(e[0] * 1500 + e[1])
    sparse = hr.from_coo(1500, 1500, key // 1500, key % 1500, np.ones(len(key)))
    assert np.array_equal(cbg.Interpret(cbg.SpParMat.from_global(grid, sparse)), hr.interpret(sparse))

    # ---- the SUMMA with empty tiles: a block-diagonal matrix leaves the off-diagonal tiles of a
    # 2 x 2 grid empty (as a converged MCL matrix does); on the host transport, whose collectives
    # are synchronous over the world, every grid row must still make the same exchanges
    bd = hr.planted()
    half = bd["n"] // 2
    r, c = bd["ir"].astype(np.int64), hr.cols_of(bd)
    same = (r < half) == (c < half)
    bd = hr.from_coo(bd["n"], bd["n"], r[same], c[same], bd["val"][same])
    if pr == 2 and pc == 2:
        assert (mine(bd)["cp"][-1] == 0) == (grid.prow != grid.pcol)
    want = cbg.MemEfficientSpGEMM(cbg.SpParMat.from_global(one, bd), cbg.SpParMat.from_global(one, bd), 1).tile.to_host()
    for exec_mode in (cbg.EXEC_PANEL, cbg.EXEC_STAGED):
        for phases in (1, 2):
            got = cbg.MemEfficientSpGEMM(cbg.SpParMat.from_global(grid, bd), cbg.SpParMat.from_global(grid, bd), phases,
                                         exec_mode=exec_mode)
            assert_tiles_bits_equal(got.tile.to_host(), mine(want))

    # ---- the loop, on both golden cases
    for p in (hr.planted(), hr.hub()):
        run_loop(cbg, grid, one, rank, p)
    grid.destroy()
    hc.allgather(0, b"x")
    print("HIPMCLOK", flush=True)


def run_loop(cbg, grid, one, rank, p):
    for ps in hr.PARAM_SETS:
        infl, h, S, R, q = ps
        kw = dict(inflation=infl, prunelimit=h, select=S, recover_num=R, recover_pct=q)
        seen = []
        labels, its = cbg.HipMCL(cbg.SpParMat.from_global(grid, p), on_iteration=lambda *a: seen.append(a), **kw)
        wl, wi = cbg.HipMCL(cbg.SpParMat.from_global(one, p), **kw)
        assert its == wi == len(seen) and np.array_equal(labels, wl), (rank, its, wi)


if __name__ == "__main__":
    main()
