#!/usr/bin/env python3
"""Compare two gfx950 assembly listings of talc_capi.hip function by function.

    hipcc --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fno-gpu-rdc --cuda-device-only -S \
          -I include -I talc_amd/csrc talc_amd/csrc/talc_capi.hip -o <side>.s        (once per side)
    tools/asm_compare.py parent.s branch.s [--changed NAME ...] > profiles/<round>/asm_compare.txt

A function's instruction sequence is its lines without comments, labels and directives; a branch target counts as
"a label".  Every function is reported with its instruction count on both sides and same / different.  For the kernels
named with --changed (substrings of the mangled name) the resource figures of both sides are printed too.  Exit status 1
when a function outside --changed differs, appears or disappears.
"""
import argparse
import re
import sys

LABEL = re.compile(r"^[.\w$]+:")
TARGET = re.compile(r"\.?LBB\d+_\d+")


def functions(path):
    """{name: [instruction, ...]} and {kernel: {figure: value}} of one listing."""
    funcs, res = {}, {}
    name, kern = None, None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            m = re.match(r"\.type\s+(\S+),@function", line)
            if m:
                name = m.group(1)
                funcs[name] = []
                continue
            if line.startswith(".Lfunc_end"):
                name = None
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
            if m:
                kern = res.setdefault(m.group(1), {})
            elif line.startswith(".end_amdhsa_kernel"):
                kern = None
            elif kern is not None:
                m = re.match(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size|accum_offset)\s+(\S+)", line)
                if m:
                    kern[m.group(1)] = m.group(2)
            if name is None or not line or line.startswith(".") or LABEL.match(line):
                continue
            funcs[name].append(TARGET.sub("a label", " ".join(line.split())))
    return funcs, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--changed", nargs="*", default=[], help="substrings of the functions that are expected to differ")
    a = ap.parse_args()
    pf, pr = functions(a.parent)
    bf, br = functions(a.branch)
    bad = 0
    print("%d functions in the parent, %d in the branch" % (len(pf), len(bf)))
    print("%-9s %8s %8s  %s" % ("", "parent", "branch", "function"))
    for name in sorted(set(pf) | set(bf)):
        expected = any(c in name for c in a.changed)
        p, b = pf.get(name), bf.get(name)
        verdict = "same" if p == b else ("changed" if expected else "DIFFERENT")
        bad += verdict == "DIFFERENT"
        print("%-9s %8s %8s  %s" % (verdict, "-" if p is None else len(p), "-" if b is None else len(b), name))
    for name in sorted(set(pr) | set(br)):
        if any(c in name for c in a.changed):
            print("\n" + name)
            for key in sorted(set(pr.get(name, {})) | set(br.get(name, {}))):
                print("  %-28s parent %6s   branch %6s" % (key, pr.get(name, {}).get(key, "-"), br.get(name, {}).get(key, "-")))
    print("\n%d function(s) outside --changed differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
