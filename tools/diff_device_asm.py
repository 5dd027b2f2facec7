#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel, wherever a kernel lives.

    for f in gpry_amd/csrc/*.hip: hipcc <CXXFLAGS of csrc/Makefile> --cuda-device-only -S f -o DIR/<name>.s
    python tools/diff_device_asm.py DIR_BEFORE DIR_AFTER

Every ``.s`` of a directory is split into function bodies (label to ``.Lfunc_end``) and ``.amdhsa_kernel`` resource blocks,
keyed by symbol; the two directories are compared symbol by symbol, so a kernel that moved to another translation unit is
compared with itself.  Local labels (``.LBB12_3``) carry a per-file function number, which is normalised away, and comments
are dropped.  Prints one line per symbol that differs or exists on one side only (``-v``: with its diff), then the counts;
exit status 1 if anything differs.
"""
import difflib
import glob
import os
import re
import sys


def split(directory):
    bodies, blocks = {}, {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        name, kernel, cur = None, None, []
        for line in open(path):
            line = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), line.split(";")[0].rstrip())
            m = re.match(r"^(_Z\w+|\w+_kernel\w*):", line)
            if m and name is None:
                name, cur = m.group(1), []
            elif name is not None and line.startswith(".Lfunc_end"):
                bodies[name] = [l for l in cur if l]
                name = None
            elif name is not None:
                cur.append(line)
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                kernel, blocks[m.group(1)] = m.group(1), []
            elif kernel is not None and ".end_amdhsa_kernel" in line:
                kernel = None
            elif kernel is not None:
                blocks[kernel].append(line.strip())
    return bodies, blocks


def main():
    before, after = split(sys.argv[1]), split(sys.argv[2])
    verbose = len(sys.argv) > 3 and sys.argv[3] == "-v"
    bad = 0
    for what, a, b in (("body", before[0], after[0]), ("amdhsa block", before[1], after[1])):
        same = 0
        for sym in sorted(set(a) | set(b)):
            if sym not in a or sym not in b:
                print(f"{what}: {sym}: only {'after' if sym not in a else 'before'}")
                bad += 1
            elif a[sym] != b[sym]:
                # the FP64 arithmetic in order, mnemonics only: a product newly fused or un-fused would show here
                f64 = [[l.split()[0] for l in x if re.match(r"\s*v_\w+_f64", l)] for x in (a[sym], b[sym])]
                verdict = "same sequence" if f64[0] == f64[1] else "same instructions, scheduled in another order" if sorted(f64[0]) == sorted(f64[1]) else "CHANGED"
                note = f"; FP64 ops: {verdict} ({len(f64[0])} -> {len(f64[1])})" if what == "body" else ""
                print(f"{what}: {sym}: DIFFERS ({len(a[sym])} -> {len(b[sym])} lines){note}")
                if verbose:
                    print("\n".join(difflib.unified_diff(a[sym], b[sym], "before", "after", lineterm="", n=2)))
                bad += 1
            else:
                same += 1
        print(f"{what}: {same} identical of {len(set(a) | set(b))}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
