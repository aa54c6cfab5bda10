#!/usr/bin/env python
"""What the compiler gave every kernel of some translation units, as one table, and the rows in which two such tables differ.

Compile the units with `-Rpass-analysis=kernel-resource-usage` added to the Makefile's CFLAGS and keep the compiler's stderr, one file per unit
or all in one.  Then
    tools/kernel_resources.py table REMARKS... > table.md     one row per kernel: SGPRs, VGPRs, AGPRs, scratch bytes per lane, occupancy
                                                              (waves per SIMD), SGPR and VGPR spills, LDS bytes per block
    tools/kernel_resources.py diff A.md B.md                  the rows that differ, and the kernels only one table has; exit status 1 if any
A kernel is named as the profiles name it: demangled, `(anonymous namespace)::` and the parameter list dropped, template arguments kept.  A kernel
that several units compile (the two copies of kamd_dev.h) is one row; its copies must agree, or the row says CONFLICT."""
import re
import shutil
import subprocess
import sys

FIELDS = [("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"),
          ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills"), ("LDS Size [bytes/block]", "LDS")]
REMARK = re.compile(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis=kernel-resource-usage\]")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):   # cut at the parameter list: the first parenthesis outside the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i]
    return name


def parse(paths):
    """{mangled name: [row, ...]} with row = the FIELDS' values, one per copy of the kernel"""
    kernels, cur = {}, None
    for path in paths:
        for line in open(path, errors="replace"):
            m = REMARK.search(line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key == "Function Name":
                cur = {}
                kernels.setdefault(val, []).append(cur)
            elif cur is not None:
                cur[key] = val
    return kernels


def table(paths):
    kernels = parse(paths)
    names = demangle(sorted(kernels))
    rows = {}
    for mangled, copies in kernels.items():
        vals = [tuple(c.get(k, "?") for k, _ in FIELDS) for c in copies]
        rows.setdefault(short(names[mangled]), []).extend(vals)
    print("| kernel | " + " | ".join(h for _, h in FIELDS) + " |")
    print("|---|" + "---:|" * len(FIELDS))
    for name in sorted(rows):
        vals = set(rows[name])
        print(f"| `{name}` | " + (" | ".join(vals.pop()) if len(vals) == 1 else " | ".join(["CONFLICT"] * len(FIELDS))) + " |")
    print(f"\n{len(rows)} kernels, {sum(len(v) for v in rows.values())} compiled copies")


def read_table(path):
    rows = {}
    for line in open(path):
        m = re.match(r"\| `(.*)` \| (.*) \|$", line.rstrip())
        if m:
            rows[m.group(1)] = m.group(2)
    return rows


def diff(a, b):
    ra, rb = read_table(a), read_table(b)
    bad = 0
    for name in sorted(set(ra) | set(rb)):
        if ra.get(name) != rb.get(name):
            bad += 1
            print(f"{name}\n  {a}: {ra.get(name, '(no such kernel)')}\n  {b}: {rb.get(name, '(no such kernel)')}")
    print(f"{len(ra)} kernels in {a}, {len(rb)} in {b}: {bad} rows differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "table":
        table(sys.argv[2:])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
