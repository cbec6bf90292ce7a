#!/usr/bin/env python3
"""Is the device code of two trees the same?  For a refactor that must not touch a kernel.

For each tree, every memo_amd/csrc/*.hip compiled with the Makefile's flags plus `-S --cuda-device-only` into a directory of its own:

    for f in memo_amd/csrc/*.hip; do hipcc --offload-arch=gfx950 <the Makefile's flags for $f> -S --cuda-device-only $f -o DIR/$(basename $f .hip).s; done
    tools/device_code_diff.py DIR_PARENT DIR_BRANCH

compares per kernel SYMBOL (a kernel may move between files): the instruction stream and the .amdhsa_ resource block.  Left out of
the comparison: comments, .loc / .file / .cfi directives, the numbers of local labels (they count the functions of a file) -- so what
remains different is a different kernel.  Exit status 1 when a kernel differs or exists on one side only."""
import glob
import os
import re
import sys


def parse(d):
    code, desc = {}, {}

    def put(table, name, body):  # (a template's kernel may be emitted by several files: the same body under one name)
        while name in table and table[name] != body:
            name += "#again"
        table[name] = body

    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        lines = open(path).read().split("\n")
        i = 0
        while i < len(lines):
            m = re.match(r"^([A-Za-z_$][\w$.]*):", lines[i])
            if not (m and any(".type\t%s,@function" % m.group(1) in l for l in lines[max(0, i - 8):i])):
                i += 1
                continue
            name, body, block = m.group(1), [], None
            i += 1
            while i < len(lines) and not re.match(r"^\.Lfunc_end\d+:", lines[i]):
                l = lines[i].split(";")[0].strip()
                i += 1
                if l.startswith(".amdhsa_kernel"):
                    block = []
                elif l.startswith(".end_amdhsa_kernel"):
                    put(desc, name, block)
                    block = None
                elif block is not None:
                    block.append(l)
                elif l and not re.match(r"^\.(loc|file|cfi_\w+)\b", l):
                    body.append(re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r"\.LBB\d+_", ".LBB_", l)))
            put(code, name, body)
    return code, desc


def main():
    (ca, da), (cb, db) = parse(sys.argv[1]), parse(sys.argv[2])
    one_side = sorted(set(ca) ^ set(cb)) + sorted(set(da) ^ set(db))
    for name in one_side:
        print("on one side only:", name)
    differing = [k for k in sorted(set(ca) & set(cb)) if ca[k] != cb[k]] + [k for k in sorted(set(da) & set(db)) if da[k] != db[k]]
    for name in differing:
        print("DIFFERENT:", name)
    print("%d kernels compared (%d lines of code, %d resource blocks): %d differing, %d on one side only"
          % (len(set(ca) & set(cb)), sum(len(ca[k]) for k in set(ca) & set(cb)), len(set(da) & set(db)), len(differing), len(one_side)))
    return 1 if differing or one_side else 0


if __name__ == "__main__":
    sys.exit(main())
