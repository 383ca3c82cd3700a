"""Writes tests/golden/bfs_<case>.npz from the reference's own top-down BFS loop, run by
tools/ref_bfs_driver.cpp (compile it by the line in its header comment).

    python tests/golden/make_bfs_golden.py <path to ref_bfs_driver>     (MPIRUN: the launcher, default mpirun)

Every case runs at 1 rank and at 4 ranks (a 2 x 2 grid) with OMP_NUM_THREADS=1.  Both runs have to
give the same parents, and those of the restatement (tests/bfs_ref.py) everywhere but at the root:
the restatement sets parents[root] = root as DirOptBFS.cpp:371 does, the reference's TopDownBFS loop
leaves the root to be found through an edge back to it (-1 for a root that nothing points back to).
A case on which the reference fails at 4 ranks is recorded from the 1-rank run alone and named in
ONE_RANK_ONLY below; the script fails when that list and what happened differ.

A fixture holds n, the stored entries A(row, col) (the edge col -> row), the roots, `parents_ref`
(one row per root, the reference's own) and `parents` (the same with parents[root] = root), the
restatement's levels, and the direction trace under the reference's rule as one string per root.

Cases
  rmat      the pattern of rmat_s10_ef16_A.npz symmetrised: 1024 vertices, 21 304 entries, 137 isolated;
            roots 0, 613 (degree 465), 5 (degree 1), the first isolated vertex (its tree is the root alone).
            The trace never returns to push.
  coretail  the same core plus a path of 40 new vertices 1024 .. 1063 hung on vertex 0, inside n = 4099
            (the rest isolated): row blocks of 2049 and 2050 on two grid rows, so no block seam falls on a
            64-bit word.  up_cutoff 1069, down_cutoff 65: every root's trace switches push -> pull, and
            roots 0, 613, 5 switch back.  The fourth root is the tail's end, 1063.
  directed  the 48 vertices of betwcent_components.npz in this feature's orientation; roots on the
            chorded cycle, the star's centre, a star leaf (reaches nothing), the isolated vertex, a corner
            of the 3 x 6 grid.
  path      130 vertices in a path, ids scrambled by a fixed permutation, both directions stored; roots
            one end (depth 129) and the middle.  The bitmap's last word has 2 bits."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bfs_ref  # noqa: E402
import hipmcl_ref as hr  # noqa: E402

# cases the reference could not run at 4 ranks (DESIGN.md says why)
ONE_RANK_ONLY = ()


def rmat_sym():
    z = np.load(os.path.join(HERE, "rmat_s10_ef16_A.npz"))
    t = {k: (int(z[k]) if k in ("m", "n") else z[k]) for k in z.files}
    r, c = t["ir"].astype(np.int64), hr.cols_of(t)
    pairs = np.unique(np.stack([np.concatenate([r, c]), np.concatenate([c, r])], 1), axis=0)
    return t["n"], pairs[:, 0], pairs[:, 1]


def case_rmat():
    n, r, c = rmat_sym()
    deg = np.bincount(c, minlength=n)
    iso = int(np.flatnonzero(deg == 0)[0])
    assert n == 1024 and len(r) == 21304 and int((deg == 0).sum()) == 137 and deg[613] == 465 and deg[5] == 1
    return n, r, c, [0, 613, 5, iso]


def case_coretail():
    n, r, c = rmat_sym()
    chain = [0] + list(range(1024, 1064))
    a, b = np.array(chain[:-1]), np.array(chain[1:])
    r, c = np.concatenate([r, a, b]), np.concatenate([c, b, a])
    assert len(r) == 21384
    return 4099, r, c, [0, 613, 5, 1063]


def case_directed():
    z = np.load(os.path.join(HERE, "betwcent_components.npz"))
    # there a stored (row, col) is the edge row -> col; here A(i, j) is j -> i
    return int(z["n"]), z["col"].astype(np.int64), z["row"].astype(np.int64), [21, 36, 37, 0, 3]


def case_path():
    perm = np.random.default_rng(130).permutation(130)
    a, b = perm[:-1], perm[1:]
    return 130, np.concatenate([a, b]), np.concatenate([b, a]), [int(perm[0]), int(perm[65])]


CASES = {"rmat": case_rmat, "coretail": case_coretail, "directed": case_directed, "path": case_path}


def run_reference(binary, n, r, c, roots, ranks):
    with tempfile.TemporaryDirectory() as d:
        mtx, out = os.path.join(d, "in.mtx"), os.path.join(d, "out.txt")
        with open(mtx, "w") as f:
            f.write("%%MatrixMarket matrix coordinate real general\n")
            f.write(f"{n} {n} {len(r)}\n")
            for i, j in zip(r.tolist(), c.tolist()):
                f.write(f"{i + 1} {j + 1} 1\n")
        cmd = [binary, mtx, out] + [str(x) for x in roots]
        if ranks > 1:
            cmd = [os.environ.get("MPIRUN", "mpirun"), "-n", str(ranks)] + cmd
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                             env=dict(os.environ, OMP_NUM_THREADS="1",  # the system libstdc++ before the MPI prefix's
                                      LD_LIBRARY_PATH="/usr/lib/x86_64-linux-gnu:" + os.environ.get("LD_LIBRARY_PATH", "")),
                             timeout=600)
        if run.returncode != 0 or not os.path.exists(out):
            return None, run.stdout[-600:]
        lines = open(out).read().split("\n")
    par, its, k = np.full((len(roots), n), -2, np.int64), [], -1
    for ln in lines:
        w = ln.split()
        if not w:
            continue
        if w[0] == "root":
            k += 1
            assert int(w[1]) == roots[k]
            its.append(int(w[3]))
        else:
            par[k, int(w[0])] = int(w[1])
    assert k == len(roots) - 1 and not np.any(par == -2)
    return par, its


def main(binary):
    failed4 = []
    for name, make in CASES.items():
        n, r, c, roots = make()
        t = hr.from_coo(n, n, r, c, np.ones(len(r)))
        one, its = run_reference(binary, n, r, c, roots, 1)
        assert one is not None, its
        four, msg = run_reference(binary, n, r, c, roots, 4)
        if four is None:
            failed4.append(name)
            print(f"{name}: the reference failed at 4 ranks: {msg.strip()[-300:]!r}")
        else:
            assert np.array_equal(one, four), name
        parents, levels, traces = one.copy(), [], []
        for k, root in enumerate(roots):
            ref = bfs_ref.bfs(t, root)
            other = np.arange(n) != root
            assert np.array_equal(ref["parents"][other], one[k][other]), (name, root)
            # the reference's root: the largest vertex of the earliest level that has an edge back to it
            # (its own loop: itself), -1 when no reached vertex has one
            back = c[(r == root) & (ref["levels"][c] >= 0)]
            first = back[ref["levels"][back] == ref["levels"][back].min()] if len(back) else back
            assert one[k][root] == (int(first.max()) if len(first) else -1), (name, root, one[k][root])
            for d in ("topdown", "bottomup"):
                assert np.array_equal(bfs_ref.bfs(t, root, d)["parents"], ref["parents"]), (name, root, d)
            assert bfs_ref.validate(t, root, ref["parents"], ref["levels"]) is None
            # the root found again re-enters the fringe once: at most one more iteration than the restatement's steps
            assert its[k] in (len(ref["steps"]), len(ref["steps"]) + 1), (name, root, its[k], len(ref["steps"]))
            parents[k][root] = root
            levels.append(ref["levels"])
            traces.append(ref["trace"])
        up, down = bfs_ref.cutoffs(t)
        if name == "coretail":
            assert (up, down) == (1069, 65), (up, down)
            for k, tr in enumerate(traces):
                assert "du" in tr, tr
                assert k == 3 or "ud" in tr, tr
        if name == "rmat":
            assert all("ud" not in tr for tr in traces), traces
        np.savez_compressed(os.path.join(HERE, f"bfs_{name}.npz"), n=np.int64(n), row=r.astype(np.int32),
                            col=c.astype(np.int32), roots=np.array(roots, np.int64), parents_ref=one, parents=parents,
                            levels=np.array(levels, np.int64), traces=np.array(traces), ranks=np.int64(1 if four is None else 4))
        print(f"{name}: n {n} entries {len(r)} roots {roots} up {up} down {down} traces {traces} "
              f"iterations {its} depth {[int(lv.max()) for lv in levels]}")
    assert tuple(failed4) == ONE_RANK_ONLY, (failed4, ONE_RANK_ONLY)


if __name__ == "__main__":
    main(sys.argv[1])
