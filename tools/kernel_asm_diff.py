#!/usr/bin/env python3
"""Is the device code of two checkouts the same?  A count and a diff of gfx950 assembly, kernel by kernel; no GPU needed.

In each checkout, for every pyfocusr_amd/csrc/*.hip (the project's flags plus a fixed compilation-unit id, with which two
builds of one file are byte-identical):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fuse-cuid=none --offload-device-only -S X.hip -o DIR/X.s
then
    python tools/kernel_asm_diff.py PARENT_DIR BRANCH_DIR
The text of a kernel is what lies between its label and the end of its function, without comments and blank lines; the
function number inside local labels (.LBB<n>_<m>) is masked, since it counts the functions that precede the kernel in its
unit.  A kernel may be emitted by several units (the library sort kernels): it is the same if the set of its texts is.
Exit status 0: the same kernel symbols, every kernel's text the same."""
import glob
import hashlib
import os
import re
import sys


def kernels(directory):
    out = {}  # symbol -> {unit: [lines]}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text = open(path).read()
        names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
        cur = None
        for line in text.split("\n"):
            m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
            if m and m.group(1) in names:
                cur = out.setdefault(m.group(1), {}).setdefault(os.path.basename(path), [])
                continue
            t = line.strip()
            if cur is None or not t or t.startswith(";") or t.startswith("//"):
                continue
            if t.startswith(".Lfunc_end"):
                cur = None
                continue
            t = re.sub(r"\s*;.*$", "", line).rstrip()
            cur.append(re.sub(r"\.(LBB|LJTI|Ltmp)\d+", r".\1N", t))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("kernel symbols: parent %d, branch %d" % (len(a), len(b)))
    print("only in parent: %s" % sorted(set(a) - set(b)))
    print("only in branch: %s" % sorted(set(b) - set(a)))
    digest = lambda units: {hashlib.sha1("\n".join(v).encode()).hexdigest() for v in units.values()}  # noqa: E731
    shared = sorted(set(a) & set(b))
    differ = [k for k in shared if digest(a[k]) != digest(b[k])]
    for k in differ:
        print("differs: %s (%s -> %s)" % (k, sorted(a[k]), sorted(b[k])))
    print("kernels whose text differs: %d of %d (%d lines compared)" % (len(differ), len(shared), sum(len(v) for k in shared for v in b[k].values())))
    for unit in sorted({u for x in (a, b) for v in x.values() for u in v}):
        na, nb = (sum(unit in v for v in x.values()) for x in (a, b))
        if na != nb:
            print("kernels emitted by %s: %d -> %d" % (unit, na, nb))
    return 0 if set(a) == set(b) and not differ else 1


if __name__ == "__main__":
    sys.exit(main())
