#!/usr/bin/env python3
"""Generate tests/golden/ fixtures by running the REFERENCE CombBLAS code.

TEST INFRASTRUCTURE ONLY -- runs in the build container (where /root/reference
exists), never on the GPU box.  Requires `make -C oracle ref` first, which
builds oracle/_ref/ref_driver from oracle/ref_driver.cpp + the reference's own
sources (see oracle/Makefile).

Outputs (all data, no reference source):
  tests/golden/golden.json      digests / totals produced by the reference
  tests/golden/*.npz            full matrices (inputs and products) for small cases

Digest definition (mirrored by tests/digest.py):
  nnz, nzc, hs = sum_e mix64(col<<32|row) mod 2^64,
  hv = sum_e mix64(col<<32|row) * mix64(bits(val)) mod 2^64, vsum = sum_e val.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
DRIVER = os.path.join(REPO, "oracle", "_ref", "ref_driver")
MPIRUN = "/opt/conda/bin/mpirun"
REF = "/root/reference"


def read_cbgt(path):
    with open(path, "rb") as f:
        magic = f.read(8)
        assert magic == b"CBGT0001", magic
        hdr = np.frombuffer(f.read(80), dtype=np.int64)
        m, n, nnz, nzc = (int(x) for x in hdr[:4])
        cp = np.frombuffer(f.read(8 * (nzc + 1)), dtype=np.int64)
        jc = np.frombuffer(f.read(4 * nzc), dtype=np.int32)
        ir = np.frombuffer(f.read(4 * nnz), dtype=np.int32)
        val = np.frombuffer(f.read(8 * nnz), dtype=np.float64)
    return dict(m=m, n=n, cp=cp, jc=jc, ir=ir, val=val, grid=hdr[4:8].tolist(), off=hdr[8:10].tolist())


def save_npz(name, t):
    np.savez_compressed(os.path.join(HERE, name), m=t["m"], n=t["n"], cp=t["cp"], jc=t["jc"], ir=t["ir"], val=t["val"])


def run(args, nprocs=1, env=None, parse=True):
    cmd = [DRIVER] + args
    if nprocs > 1:
        cmd = [MPIRUN, "-n", str(nprocs)] + cmd
    e = dict(os.environ)
    e.setdefault("OMP_NUM_THREADS", "8")
    if env:
        e.update(env)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, env=e).stdout
    recs = []
    if not parse:  # (a digest of non-finite values prints vsum as nan: not JSON)
        return recs
    for line in out.splitlines():
        line = line.strip()
        if line.startswith("{"):
            recs.append(json.loads(line))
    return recs


def tagged(recs, tag):
    for r in recs:
        if r.get("tag") == tag:
            d = dict(r)
            d.pop("tag")
            return d
    raise KeyError(tag)


def main():
    if not os.path.exists(DRIVER):
        sys.exit("build the reference driver first: make -C oracle ref")
    gold = {"_doc": __doc__.strip().splitlines()[0], "rmat": {}, "files": {}}
    tmp = tempfile.mkdtemp(prefix="cbg_golden_")

    # ---- bundled small inputs (configs[0]: MultTest plumbing, fp-tolerance KAT) ----
    files = {
        "sevenvertex": ("readmm", f"{REF}/ReleaseTests/sevenvertex.mtx", None),
        "small_nonsym": ("readtriples", f"{REF}/ReleaseTests/small_nonsym.mtx", None),
        "largeseq": ("readtriples", f"{REF}/largeseq/input1_0", f"{REF}/largeseq/input2_0"),
    }
    for name, (mode, fa, fb) in files.items():
        entry = {}
        pa = os.path.join(tmp, name + "_A.cbgt")
        entry["A"] = tagged(run([mode, fa, pa]), "A")
        A = read_cbgt(pa)
        save_npz(f"{name}_A.npz", A)
        pb = pa
        if fb is not None:
            pb = os.path.join(tmp, name + "_B.cbgt")
            entry["B"] = tagged(run([mode, fb, pb]), "A")
            save_npz(f"{name}_B.npz", read_cbgt(pb))
        else:
            # A*A with B a deep copy of A (aliasing is forbidden, ParFriends.h:172-178)
            pb = os.path.join(tmp, name + "_B.cbgt")
            with open(pa, "rb") as s, open(pb, "wb") as d:
                d.write(s.read())
        for sr in ("plus", "minplus"):
            for algo in ("local", "heap", "doublebuff", "synch"):
                pc = os.path.join(tmp, f"{name}_C_{algo}_{sr}.cbgt")
                recs = run(["mult", algo, sr, pa, pb, pc])
                entry[f"C_{algo}_{sr}"] = tagged(recs, f"C_{algo}_{sr}")
                if algo in ("local", "doublebuff"):
                    save_npz(f"{name}_C_{algo}_{sr}.npz", read_cbgt(pc))
            # distributed 2x2 grid, same product (reference's square-grid SUMMA)
            if name != "sevenvertex":  # 7x7 with 4 ranks is fine for GEMM; keep the set small
                for algo in ("doublebuff", "synch"):
                    recs = run(["mult", algo, sr, pa, pb, "-"], nprocs=4)
                    entry[f"C_{algo}_{sr}_p4"] = tagged(recs, f"C_{algo}_{sr}")
        gold["files"][name] = entry
        print(name, "done", flush=True)

    # ---- R-MAT A*A (Graph500 Kronecker, SEED default 0xDECAFBAD) ----
    scales = [int(s) for s in os.environ.get("GOLD_SCALES", "8,10,12,14,16,18").split(",")]
    for scale in scales:
        ef = 16
        key = f"s{scale}_ef{ef}"
        entry = {}
        pa = os.path.join(tmp, key + "_A.cbgt")
        recs = run(["gen", str(scale), str(ef), pa])
        entry["A"] = tagged(recs, "A")
        entry["loops_removed"] = tagged(recs, "gen_loops_removed")["value"]
        A = read_cbgt(pa)
        pb = os.path.join(tmp, key + "_B.cbgt")
        with open(pa, "rb") as s, open(pb, "wb") as d:
            d.write(s.read())
        if scale <= 10:
            save_npz(f"rmat_{key}_A.npz", A)
        algos = ("local", "heap", "doublebuff", "synch") if scale <= 16 else ("local", "synch", "doublebuff")
        for algo in algos:
            for sr in (("plus", "minplus") if algo == "local" else ("plus",)):
                pc = os.path.join(tmp, f"{key}_C_{algo}_{sr}.cbgt") if (scale <= 10 and algo == "local") else "-"
                recs = run(["mult", algo, sr, pa, pb, pc])
                entry[f"C_{algo}_{sr}"] = tagged(recs, f"C_{algo}_{sr}")
                entry[f"time_{algo}_{sr}"] = tagged(recs, f"time_{algo}")["seconds"]
                if pc != "-":
                    save_npz(f"rmat_{key}_C_{algo}_{sr}.npz", read_cbgt(pc))
        if scale <= 14:
            recs = run(["mult", "doublebuff", "plus", pa, pb, "-"], nprocs=4)
            entry["C_doublebuff_plus_p4"] = tagged(recs, "C_doublebuff_plus")
        entry["symbolic"] = tagged(run(["symbolic", pa, pb]), "symbolic")
        gold["rmat"][key] = entry
        print(key, "done", flush=True)
        with open(os.path.join(HERE, "golden.json"), "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)

    big_scales(gold, tmp, os.environ.get("GOLD_BIG", "20x16,20x8,22x16,22x8"))
    with open(os.path.join(HERE, "golden.json"), "w") as f:
        json.dump(gold, f, indent=1, sort_keys=True)
    multtest_fixture()


def big_scales(gold, tmp, spec):
    """large scales: inputs + symbolic totals only (C does not fit this host)"""
    big = [tuple(int(x) for x in s.split("x")) for s in spec.split(",") if s]
    for scale, ef in big:
        key = f"s{scale}_ef{ef}"
        entry = {}
        pa = os.path.join(tmp, key + "_A.cbgt")
        recs = run(["gen", str(scale), str(ef), pa])
        entry["A"] = tagged(recs, "A")
        entry["loops_removed"] = tagged(recs, "gen_loops_removed")["value"]
        entry["symbolic"] = tagged(run(["symbolic", pa, pa]), "symbolic")
        os.remove(pa)
        gold["rmat"][key] = entry
        print(key, "done", flush=True)
        with open(os.path.join(HERE, "golden.json"), "w") as f:
            json.dump(gold, f, indent=1, sort_keys=True)


def multtest_fixture():
    """ReleaseTests/MultTest inputs: the reference's bundled sevenvertex.mtx (data
    file, copied) and CControl = the reference's product of it with itself
    (sevenvertex_C_local_plus.npz above), written as Matrix Market."""
    import shutil
    shutil.copyfile(f"{REF}/ReleaseTests/sevenvertex.mtx", os.path.join(HERE, "sevenvertex.mtx"))
    d = np.load(os.path.join(HERE, "sevenvertex_C_local_plus.npz"))
    cols = np.repeat(d["jc"].astype(np.int64), np.diff(d["cp"]))
    with open(os.path.join(HERE, "sevenvertex_C.mtx"), "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{int(d['m'])} {int(d['n'])} {len(d['ir'])}\n")
        for r, c, v in zip(d["ir"], cols, d["val"]):
            f.write(f"{int(r) + 1} {int(c) + 1} {float(v)!r}\n")


def write_cbgt(path, t):
    """a host tile as a 1x1-grid .cbgt (the mirror of read_cbgt)"""
    nnz, nzc = len(t["ir"]), len(t["jc"])
    with open(path, "wb") as f:
        f.write(b"CBGT0001")
        f.write(np.array([t["m"], t["n"], nnz, nzc, 1, 1, 0, 0, 0, 0], np.int64).tobytes())
        f.write(np.ascontiguousarray(t["cp"], np.int64).tobytes())
        f.write(np.ascontiguousarray(t["jc"], np.int32).tobytes())
        f.write(np.ascontiguousarray(t["ir"], np.int32).tobytes())
        f.write(np.ascontiguousarray(t["val"], np.float64).tobytes())


def special_fixture():
    """signed zeros, infinities, subnormals, DBL_MAX through the reference's local
    multiplies: a 60x40 A and a 40x30 B with the f64 palette (plus-times) and the
    min-plus palette of tests/helpers.py, C by LocalHybridSpGEMM; the heap kernel
    must give the same bits (NaN by position), or the case is order dependent and
    no fixture is written."""
    sys.path.insert(0, os.path.dirname(HERE))
    from helpers import assert_tiles_bits_equal, rand_tile, with_palette
    tmp = tempfile.mkdtemp(prefix="cbg_special_")
    rng = np.random.default_rng(2024)
    A0, B0 = rand_tile(rng, 60, 40, 0.3), rand_tile(rng, 40, 30, 0.3)
    for sr, palette in (("plus", "f64"), ("minplus", "minplus")):
        A, B = with_palette(A0, B0, palette, rng)
        pa, pb = os.path.join(tmp, f"{sr}_A.cbgt"), os.path.join(tmp, f"{sr}_B.cbgt")
        write_cbgt(pa, A)
        write_cbgt(pb, B)
        C = {}
        for algo in ("local", "heap"):
            pc = os.path.join(tmp, f"{sr}_C_{algo}.cbgt")
            run(["mult", algo, sr, pa, pb, pc], parse=False)
            C[algo] = read_cbgt(pc)
        assert_tiles_bits_equal(C["heap"], C["local"])
        save_npz(f"special_{sr}_A.npz", A)
        save_npz(f"special_{sr}_B.npz", B)
        save_npz(f"special_{sr}_C_local.npz", C["local"])
        print("special", sr, "nnz(C) =", len(C["local"]["ir"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "special":
        special_fixture()
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "big":
        # add large-scale symbolic totals to the existing golden.json, e.g. `big 24x16`
        with open(os.path.join(HERE, "golden.json")) as f:
            g = json.load(f)
        big_scales(g, tempfile.mkdtemp(prefix="cbg_golden_"), sys.argv[2])
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "multtest":
        multtest_fixture()
    else:
        main()
