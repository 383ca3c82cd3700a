"""cbg_grid_betwcent (csrc/cbg_grid_algos.cpp, kernels in csrc/cbg_ewise.hip) against the fixtures of
tests/golden/make_betwcent_golden.py: the reference's own BetwCent agrees with the exact
rational Brandes of tests/betwcent_ref.py there, and the device has to agree with the exact
values within

    |bc_got[v] - bc_exact[v]| <= K * 2^-52 * (bc_exact[v] + nroots),
    K = D * (degree + 4) + nroots + batches + 2

(everything up to the final subtraction is a sum of positive terms; K counts the roundings on
the longest chain: D levels of at most `degree` additions and four products or quotients each,
nroots row-sum additions, one addition per batch, the subtraction).  One lost path would move a
value by at least 1 / sigma_max, above 1e-7 for every fixture.  Level sizes are exact."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import betwcent_ref as br
from betwcent_worker import CASES, bound, load_case
from test_gpu_hipmcl import _self_grid
from test_multiprocess import free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture
def grid(cbg):
    g = _self_grid(cbg)
    yield g
    g.destroy()


@functools.lru_cache(maxsize=None)
def _exact(name, batch, nroots=None):
    z, a, _ = load_case(name)
    return br.brandes(a, z["roots"][:nroots].tolist(), batch)


def _run(cbg, grid, name, batch, give_at=False, nroots=None):
    z, a, at = load_case(name)
    A = cbg.SpParMat.from_global(grid, a)
    AT = cbg.SpParMat.from_global(grid, at) if give_at else None
    seen = []
    bc = cbg.BetwCent(A, z["roots"][:nroots], batch, AT=AT, on_level=lambda b, lv, nnz: seen.append((b, lv, nnz)))
    return z, bc, seen, cbg.betwcent_stats()


@pytest.mark.parametrize("name", CASES)
def test_betwcent_fixture(cbg, grid, name):
    z0 = load_case(name)[0]
    batch = int(z0["batch"])
    z, bc, seen, st = _run(cbg, grid, name, batch)
    nroots = len(z["roots"])
    nb = -(-nroots // batch)
    err = np.abs(bc - z["bc_exact"])
    bnd = bound(z, nroots, nb)
    print(name, "max error", float(err.max()), "smallest bound", float(bnd.min()), "against the reference",
          float(np.abs(bc - z["bc_ref"]).max()))
    assert np.all(err <= bnd), (float(err.max()), float(bnd.min()))
    assert np.all(np.abs(bc - z["bc_ref"]) <= 2 * bnd)  # the reference's own run is within the bound as well
    want = _exact(name, batch)
    assert [float(x) for x in want["bc"]] == z["bc_exact"].tolist()
    assert seen == [(b, k + 1, s) for b, lv in enumerate(want["levels"]) for k, s in enumerate(lv)]
    counts = np.cumsum(np.concatenate([[0], z["level_counts"]]))
    assert [s for _, _, s in seen] == z["level_sizes"].tolist() and len(seen) == counts[-1]
    assert st["batches"] == nb and st["levels"] == len(seen) and st["deepest"] == max(lv for _, lv, _ in seen)
    assert st["fringe_entries"] == sum(s for _, _, s in seen) and st["ms_total"] > 0
    assert max(lv for _, lv, _ in seen) == int(z["depth"])


@pytest.mark.parametrize("name", CASES)
def test_betwcent_batch_sizes(cbg, grid, name):
    """one root at a time, a batch that divides nroots into several batches, one that does not, and all at
    once.  The components fixture has 17 roots, a prime: its first 16 are taken here (the isolated root and
    the two-vertex component among them), the exact values recomputed for them."""
    z0 = load_case(name)[0]
    nroots = len(z0["roots"]) // 4 * 4
    batches = [1, 4, 3, nroots + 83]
    assert nroots in (8, 16) and nroots % 3 != 0
    exact = np.array([float(x) for x in _exact(name, nroots, nroots)["bc"]])
    got, bnds = [], []
    for i, batch in enumerate(batches):
        z, bc, seen, st = _run(cbg, grid, name, batch, give_at=bool(i % 2), nroots=nroots)
        nb = -(-nroots // batch)
        K = br.bound_factor(int(z["depth"]), int(z["degree"]), nroots, nb)
        bnds.append(K * 2.0 ** -52 * (exact + nroots))
        assert np.all(np.abs(bc - exact) <= bnds[-1]), (batch, float(np.abs(bc - exact).max()))
        want = _exact(name, batch, nroots)["levels"]
        assert seen == [(b, k + 1, s) for b, lv in enumerate(want) for k, s in enumerate(lv)], batch
        assert st["batches"] == nb
        got.append(bc)
    widest = np.max(bnds, axis=0)
    for i in range(len(got)):
        for j in range(i):
            assert np.all(np.abs(got[i] - got[j]) <= widest), (batches[i], batches[j])


@pytest.mark.parametrize("name", CASES)
def test_forward_phase_from_the_pieces(cbg, grid, name):
    """the forward sweep composed from SubsRef, PSpGEMM, += and EWiseMult: the path counts are
    the exact ones"""
    z, a, at = load_case(name)
    roots = z["roots"]
    n = a["n"]
    AT = cbg.SpParMat.from_global(grid, at)
    fringe = AT.SubsRef(None, roots)
    nsp = cbg.SpParMat.from_global(grid, br.hr.from_coo(n, len(roots), roots, np.arange(len(roots)), np.ones(len(roots))))
    levels = 0
    while fringe.getnnz() > 0:
        nsp += fringe
        fringe = cbg.EWiseMult(cbg.PSpGEMM(AT, fringe), nsp, True)
        assert fringe.tile.digest()["unsorted"] == 0
        levels += 1
    h = nsp.tile.to_host()
    got = np.zeros((n, len(roots)))
    got[h["ir"], br.hr.cols_of(h)] = h["val"]
    want = np.array(_exact(name, len(roots))["sigma"], np.float64).T
    np.testing.assert_array_equal(got, want)
    assert levels == int(z["depth"]) and want.max() == float(z["sigma_max"])


def test_betwcent_candidates(cbg, grid):
    for name in CASES:
        z, _, at = load_case(name)
        AT = cbg.SpParMat.from_global(grid, at)
        np.testing.assert_array_equal(cbg.betwcent_candidates(AT, len(z["ref_roots"])), z["ref_roots"])
    assert len(cbg.betwcent_candidates(AT, 10 ** 6)) == int((np.bincount(z["row"], minlength=int(z["n"])) > 0).sum()) == 36


def test_betwcent_ignores_values_and_loops(cbg, grid):
    """stored values and loops do not change bc (the library's documented deviation from the reference)"""
    z, a, _ = load_case("components")
    n = a["n"]
    rng = np.random.default_rng(5)
    row = np.concatenate([z["row"], np.arange(0, n, 3)])
    col = np.concatenate([z["col"], np.arange(0, n, 3)])
    noisy = br.hr.from_coo(n, n, row, col, rng.uniform(-4, 4, len(row)))
    A = cbg.SpParMat.from_global(grid, noisy)
    before = A.tile.digest()
    bc = cbg.BetwCent(A, z["roots"], 4)
    assert A.tile.digest()["hs"] == before["hs"] and A.tile.digest()["hv"] == before["hv"]  # A is left as it was
    assert np.all(np.abs(bc - z["bc_exact"]) <= bound(z, len(z["roots"]), 5))
    np.testing.assert_array_equal(cbg.BetwCent(A, [], 4), np.zeros(n))


def test_on_level_exception_is_raised_after_the_call(cbg, grid):
    z, a, _ = load_case("components")
    A = cbg.SpParMat.from_global(grid, a)
    calls = []

    def boom(b, level, nnz):
        calls.append(level)
        raise ZeroDivisionError("from on_level")

    with pytest.raises(ZeroDivisionError):
        cbg.BetwCent(A, z["roots"], 4, on_level=boom)
    assert len(calls) == int(z["level_counts"].sum())  # the collective ran to its end


def test_betwcent_check_driver(cbg, tmp_path):
    """tools/betwcent_check (the C++ mirror header, the reference's command line) on the lattice:
    the file holds AT, the roots are the reference's, the written bc is within the bound"""
    exe = os.path.join(os.path.dirname(HERE), "tools", "betwcent_check")
    if not os.path.exists(exe):
        pytest.fail("tools/betwcent_check is not built (make -C combblas-spmm-test_amd drivers)")
    z, a, at = load_case("lattice")
    cbg.write_mm(str(tmp_path / "input.mtx"), at)
    out = tmp_path / "bc.txt"
    run = subprocess.run([exe, str(tmp_path), "3", "4", str(out)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "BETWCENTCHECK OK" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    assert "EWiseMult + SetDifference: ok" in run.stdout and "roots 8 batches 2 levels 40" in run.stdout, run.stdout[-1500:]
    lines = out.read_text().split("\n")
    assert lines[0].split() == ["144", "1", "144"]
    bc = np.array([float(ln.split()[2]) for ln in lines[1:] if ln.strip()])
    assert [int(ln.split()[0]) for ln in lines[1:] if ln.strip()] == list(range(1, 145))
    assert np.all(np.abs(bc - z["bc_exact"]) <= bound(z, 8, 2))


# ---------------------------------------------------------------------------
# several ranks
# ---------------------------------------------------------------------------
def _launch(nproc, args, timeout=300):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.join(HERE, "betwcent_worker.py")] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, OMP_NUM_THREADS="1"))
    out = r.stdout + r.stderr
    errs = [ln for ln in out.splitlines() if "CbgError" in ln or "[cbg]" in ln or "AssertionError" in ln]
    return r.returncode, "\n".join(errs[:16]) + "\n" + out


@pytest.mark.parametrize("grid_shape", [(2, 1), (1, 2), (2, 2)])
def test_betwcent_multirank_host_transport(grid_shape):
    """bc identical on all ranks and within the bound; AT handed over on 2 x 1 and 1 x 2 (and the
    NOTSQUARE error without it agreed), left to the library on 2 x 2"""
    rc, out = _launch(grid_shape[0] * grid_shape[1], ["gpu", str(grid_shape[0]), str(grid_shape[1])])
    assert rc == 0 and out.count("BETWCENTOK") == grid_shape[0] * grid_shape[1], out[:1500] + out[-3000:]


def test_betwcent_multirank_rccl():
    rc, out = _launch(2, ["rccl", "2", "1"])
    assert rc == 0 and out.count("BETWCENTOK") == 2 and "transport rccl" in out, out[:1500] + out[-3000:]
