#!/usr/bin/env python3
"""Compare the device assembly of two builds of the library, unit by unit.

    make -C saprobe-alac_amd/csrc asm UNIT=k_dec16q      (once per unit and per build: leaves <unit>-hip-amdgcn-amd-amdhsa-gfx950.s)
    tools/isa_compare.py DIR_A DIR_B [--diff-dir DIR]

Each .s is stripped of comments (';' to the end of the line), blank lines and the per-compilation __hip_cuid_* symbol; then
the two sides are compared and the instruction lines of every kernel counted. With --diff-dir, the unified diff of each unit
that differs is written to DIR/isa_diff_<unit>.txt."""
import argparse
import difflib
import glob
import os
import re

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def stripped(path):
    out = []
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        if line.strip() and "__hip_cuid_" not in line:
            out.append(line)
    return out


def kernel_counts(lines):
    """{kernel: instruction lines}: what stands between a function's label and its .Lfunc_end, labels and directives aside."""
    funcs = {m.group(1) for m in (re.match(r"\s*\.type\s+(\S+),@function", s) for s in lines) if m}
    counts, cur = {}, None
    for s in lines:
        t = s.strip()
        if t.endswith(":"):
            if t[:-1] in funcs:
                cur, counts[t[:-1]] = t[:-1], 0
            elif t.startswith(".Lfunc_end"):
                cur = None
        elif cur is not None and not t.startswith("."):
            counts[cur] += 1
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--diff-dir")
    args = ap.parse_args()
    differ = 0
    for pa in sorted(glob.glob(os.path.join(args.dir_a, "*" + SUFFIX))):
        unit = os.path.basename(pa)[:-len(SUFFIX)]
        pb = os.path.join(args.dir_b, unit + SUFFIX)
        if not os.path.exists(pb):
            print("%-12s only in %s" % (unit, args.dir_a))
            continue
        a, b = stripped(pa), stripped(pb)
        same = a == b
        differ += not same
        print("%-12s %s" % (unit, "identical" if same else "DIFFERS"))
        ca, cb = kernel_counts(a), kernel_counts(b)
        for k in sorted(set(ca) | set(cb)):
            print("    %-60s %8s %8s" % (k, ca.get(k, "-"), cb.get(k, "-")))
        if not same and args.diff_dir:
            os.makedirs(args.diff_dir, exist_ok=True)
            with open(os.path.join(args.diff_dir, "isa_diff_%s.txt" % unit), "w") as f:
                f.writelines(s + "\n" for s in difflib.unified_diff(a, b, "a/" + unit, "b/" + unit, lineterm=""))
    return 1 if differ else 0


if __name__ == "__main__":
    raise SystemExit(main())
