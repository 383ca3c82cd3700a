#!/usr/bin/env python3
"""Kernel resources from the compiler's remarks (hipcc ... -Rpass-analysis=kernel-resource-usage 2> LOG).

  tools/kernel_resources.py LOG            one line per kernel: name, sgpr, vgpr, agpr, scratch, occupancy, lds
  tools/kernel_resources.py BASE HEAD      the kernels that differ (or exist on one side only), and a summary;
                                           exit status 1 when the kernel sets, scratch, occupancy or LDS differ

Names are demangled (llvm-cxxfilt or c++filt, whichever is found; mangled otherwise).  Reads nothing but the logs."""
import collections
import re
import shutil
import subprocess
import sys

FIELDS = (("sgpr", "TotalSGPRs"), ("vgpr", "VGPRs"), ("agpr", "AGPRs"), ("scratch", "ScratchSize [bytes/lane]"),
          ("occ", "Occupancy [waves/SIMD]"), ("lds", "LDS Size [bytes/block]"))
HARD = ("scratch", "occ", "lds")  # what may not move
REMARK = re.compile(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]\s*$")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool or not names:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    out = out.splitlines()
    return out if len(out) == len(names) else list(names)


def parse(path):
    """{demangled kernel name: {field: int}}"""
    keys = {label: key for key, label in FIELDS}
    mangled, rows, cur = [], [], None
    with open(path, errors="replace") as f:
        for line in f:
            m = REMARK.search(line)
            if not m:
                continue
            label, value = m.group(1).strip(), m.group(2)
            if label == "Function Name":
                cur = {}
                mangled.append(value)
                rows.append(cur)
            elif cur is not None and label in keys:
                cur[keys[label]] = int(value)
    return dict(zip(demangle(mangled), rows))


def line(name, r):
    return " ".join("%s=%d" % (k, r.get(k, -1)) for k, _ in FIELDS) + "  " + name


def family(name):
    """the kernel's name without return type, namespace, template and function arguments"""
    head = re.split(r"[<(]", name, 1)[0]
    return head.split()[-1].split("::")[-1] if head.split() else name


def main(argv):
    if len(argv) == 2:
        table = parse(argv[1])
        print("\n".join(line(name, table[name]) for name in sorted(table)))
        fam = collections.Counter(family(n) for n in table)
        print("# %d kernels: %s" % (len(table), ", ".join("%s %d" % kv for kv in sorted(fam.items()))), file=sys.stderr)
        return 0
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    base, head = parse(argv[1]), parse(argv[2])
    bad = 0
    for name in sorted(set(base) | set(head)):
        b, h = base.get(name), head.get(name)
        if b is None or h is None:
            print("%s %s" % ("+" if b is None else "-", name))
            bad += 1
        elif b != h:
            hard = [k for k in HARD if b.get(k) != h.get(k)]
            bad += bool(hard)
            print("%s %s\n    base %s\n    head %s" % ("!" if hard else "~", name, line("", b), line("", h)))
    print("# base %d kernels, head %d; %d with a missing twin or a change of %s" % (len(base), len(head), bad, "/".join(HARD)),
          file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
