"""The BFS restatement (tests/bfs_ref.py) against the fixtures of tests/golden/make_bfs_golden.py, which
hold the parents of the reference's own top-down loop (CPU-only).  The restatement sets
parents[root] = root as DirOptBFS.cpp:371 does; the reference's TopDownBFS loop leaves the root to
be found through an edge back to it, so the two are compared everywhere but at the root."""
import numpy as np
import pytest

import bfs_ref
from bfs_worker import CASES, load_case


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    z, a = load_case(name)
    n = a["n"]
    for k, root in enumerate(z["roots"].tolist()):
        other = np.arange(n) != root
        got = {d: bfs_ref.bfs(a, root, d) for d in ("auto", "topdown", "bottomup")}
        for d, r in got.items():
            assert np.array_equal(r["parents"][other], z["parents_ref"][k][other]), (root, d)
            assert r["parents"][root] == root and np.array_equal(r["parents"], z["parents"][k])
            assert np.array_equal(r["levels"], z["levels"][k]), (root, d)
            assert bfs_ref.validate(a, root, r["parents"], r["levels"]) is None
        assert got["auto"]["trace"] == str(z["traces"][k])
        assert set(got["topdown"]["trace"]) == {"d"} and set(got["bottomup"]["trace"]) == {"u"}
        st = got["auto"]["stats"]
        assert st["reached"] == int((z["parents"][k] >= 0).sum()) and st["levels"] == int(z["levels"][k].max())
        assert st["edges"] == int(bfs_ref.col_lengths(a)[z["parents"][k] >= 0].sum())


def test_fixture_shapes_and_traces():
    z, a = load_case("rmat")
    deg = bfs_ref.col_lengths(a)
    assert a["n"] == 1024 and len(a["ir"]) == 21304 and int((deg == 0).sum()) == 137
    assert z["roots"].tolist()[:3] == [0, 613, 5] and deg[613] == 465 and deg[5] == 1 and deg[z["roots"][3]] == 0
    assert int((z["parents"][3] >= 0).sum()) == 1  # the isolated root's tree is the root alone
    assert [str(t) for t in z["traces"]] == ["duuu", "duuu", "dduuuu", "d"]  # never back to push
    z, a = load_case("coretail")
    assert a["n"] == 4099 and len(a["ir"]) == 21384 and bfs_ref.cutoffs(a) == (1069, 65)
    assert z["roots"].tolist() == [0, 613, 5, 1063]
    tr = [str(t) for t in z["traces"]]
    assert tr == ["duuu" + "d" * 37, "duu" + "d" * 39, "dduuu" + "d" * 39, "d" * 41 + "uuu"]
    assert all("du" in t for t in tr) and all("ud" in t for t in tr[:3])
    z, a = load_case("path")
    assert a["n"] == 130 and a["n"] % 64 == 2 and int(z["levels"][0].max()) == 129 and int(z["levels"][1].max()) == 65
    z, a = load_case("directed")
    assert a["n"] == 48 and int((z["parents"][2] >= 0).sum()) == 1 and int((z["parents"][3] >= 0).sum()) == 1


def test_cutoff_overrides_change_only_the_trace():
    z, a = load_case("rmat")
    base = bfs_ref.bfs(a, 0)
    forced = bfs_ref.bfs(a, 0, up_cutoff=0, down_cutoff=10 ** 6)
    assert forced["trace"] != base["trace"] and "ud" in forced["trace"]
    assert np.array_equal(forced["parents"], base["parents"]) and np.array_equal(forced["levels"], base["levels"])


def test_validator_rejects_broken_trees():
    z, a = load_case("coretail")
    root = 613
    r = bfs_ref.bfs(a, root)
    p, lv = r["parents"], r["levels"]
    assert bfs_ref.validate(a, root, p, lv) is None
    # a wrong parent: a vertex of the same level is no neighbour on the level before
    v = int(np.flatnonzero(lv == 2)[0])
    bad = p.copy()
    bad[v] = int(np.flatnonzero((lv == 1) & (np.arange(a["n"]) != p[v]))[-1])
    stored = set(zip(bfs_ref.hr.cols_of(a).tolist(), a["ir"].tolist()))
    assert (int(bad[v]), v) not in stored
    assert "no stored edge from its parent" in bfs_ref.validate(a, root, bad, lv)
    # a skipped level
    bad = lv.copy()
    bad[v] = 3
    assert "plus one" in bfs_ref.validate(a, root, p, bad)
    # a reached vertex marked unreached (the tail's end: nothing hangs on it)
    bp, bl = p.copy(), lv.copy()
    bp[1063], bl[1063] = -1, -1
    assert "leaves the reached set" in bfs_ref.validate(a, root, bp, bl)
    # the root
    bp = p.copy()
    bp[root] = -1
    assert "root" in bfs_ref.validate(a, root, bp, lv)
    # an edge that spans two levels: lift a whole subtree's level by one
    bl = lv.copy()
    deep = lv == lv.max()
    bl[deep] += 1
    assert bfs_ref.validate(a, root, p, bl) is not None


def test_pull_counts_and_push_agree():
    rng = np.random.default_rng(3)
    m, n = 60, 40
    keep = rng.random((m, n)) < 0.15
    r, c = np.nonzero(keep)
    t = bfs_ref.hr.from_coo(m, n, r, c, np.ones(len(r)))
    x = np.sort(rng.choice(n, 9, replace=False))
    yi, yv = bfs_ref.spmspv_max(t, x)
    pi, pv, read = bfs_ref.pull_max(t, x)
    assert np.array_equal(yi, pi) and np.array_equal(yv, pv)
    want = 0
    for i in range(m):
        cols = np.flatnonzero(keep[i])[::-1]
        hit = np.flatnonzero(np.isin(cols, x))
        want += (hit[0] + 1) if len(hit) else len(cols)
    assert read == want
    assert np.array_equal(yv, [max(j for j in x if keep[i, j]) for i in yi])
