"""Kernel-by-kernel comparison of the device assembly of two builds of the same .hip files.

  for f in norm norm_ex prelu; do hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S csrc/$f.hip -o <dir>/$f.s; done
  (once in a checkout of the parent commit, once here; every *.s of the two directories is read)
  python tools/isa_diff.py <parent dir> <new dir> [--rename OLD=NEW ...] > profiles/<name>_isa.txt

One line per kernel: VGPRs, LDS bytes and scratch bytes of both builds, and whether the instruction streams are identical after
symbol names and local label numbers are normalised and the two factors of an integer multiply (v_mul_lo_u32, v_mad_u64_u32) are
put in a fixed order: say so next to a table made with this. --rename matches a kernel of the parent with a differently named
kernel of the new build (demangled names, a substring is replaced). --diff appends the unified diff of the normalised instruction
streams of every kernel that is not identical. Exit status 1 when a kernel of the new build has scratch, more VGPRs
or another LDS size than its parent, or has no parent.
"""
import argparse
import difflib
import re
import subprocess
import sys
from pathlib import Path


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    # "void name<args>(params)" -> "name<args>"
    return [re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", o.strip())) for o in out[:len(names)]]


def kernels(path):
    text = Path(path).read_text()
    found = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
        sym = m.group(1)
        start = text.index("\n%s:" % sym) + 1
        end = text.index("s_endpgm", start)
        body = []
        for line in text[start:end].split("\n")[1:]:
            line = line.split(";")[0].strip()
            if not line:
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)           # local labels carry the function's index in the file
            line = re.sub(r"\b_Z\w+", "SYM", line)               # LDS arrays and the like are named after the kernel
            m2 = re.match(r"(v_mul_lo_u32 \S+ |v_mad_u64_u32 \S+ \S+ )(\S+), (\S+?)(,.*)?$", line)
            if m2:                                               # a * b = b * a: the two factors in a fixed order
                lo, hi = sorted(m2.group(2, 3))
                line = "%s%s, %s%s" % (m2.group(1), lo, hi, m2.group(4) or "")
            body.append(line)
        info = text[text.index(".end_amdhsa_kernel", m.end()):]
        num = lambda key: int(re.search(r"^; %s: (\d+)" % key, info, re.M).group(1))
        found[sym] = dict(vgpr=num("TotalNumVgprs"), lds=num("LDSByteSize"), scratch=num("ScratchSize"), body=body)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], help="OLD=NEW substring of a demangled kernel name")
    ap.add_argument("--diff", action="store_true", help="append the instruction diff of every kernel that is not identical")
    args = ap.parse_args()
    bad = 0
    print("%-78s %9s %13s %9s %s" % ("kernel", "VGPRs p/n", "LDS p/n", "scratch", "identical"))
    a, b = {}, {}
    for d, into in ((args.parent, a), (args.new, b)):
        for f in sorted(Path(d).glob("*.s")):
            k = kernels(f)
            into.update(zip(demangle(list(k)), k.values()))
    for r in args.rename:
        old, new = r.split("=")
        a = {k.replace(old, new): v for k, v in a.items()}
    print("# %d kernels (parent %d)" % (len(b), len(a)))
    for name in sorted(b):
        kb, ka = b[name], a.get(name)
        if ka is None:
            print("%-78s %9s %13s %9d %s" % (name, "-/%d" % kb["vgpr"], "-/%d" % kb["lds"], kb["scratch"], "no parent"))
            bad += 1
            continue
        same = ka["body"] == kb["body"]
        print("%-78s %9s %13s %9s %s" % (name, "%d/%d" % (ka["vgpr"], kb["vgpr"]), "%d/%d" % (ka["lds"], kb["lds"]),
                                         "%d/%d" % (ka["scratch"], kb["scratch"]), "yes" if same else "no"))
        bad += kb["scratch"] != 0 or kb["vgpr"] > ka["vgpr"] or kb["lds"] != ka["lds"]
    for name in sorted(set(a) - set(b)):
        print("%-78s only in the parent" % name)
    if args.diff:
        for name in sorted(b):
            if name in a and a[name]["body"] != b[name]["body"]:
                print("\n## %s" % name)
                print("\n".join(difflib.unified_diff(a[name]["body"], b[name]["body"], "parent", "new", n=1, lineterm="")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
