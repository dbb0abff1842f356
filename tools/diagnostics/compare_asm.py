#!/usr/bin/env python3
"""Function-by-function comparison of two device assembly listings (`make -C raytracer.glsl_amd/csrc asm` on two trees): which functions
exist on one side only and, for each function whose instructions differ, its line counts and how many lines differ.
`;` comments, the numbers of `.LBB<n>_<m>` / `.Lfunc_end<n>` labels and each function's own name are stripped first.  A report, not a
gate: it exits 0 either way.

    compare_asm.py parent.s new.s [--rename REGEX REPLACEMENT ...]      (a rename is applied to the function names of both files)"""
import argparse
import difflib
import re


def functions(path, renames):
    """{name: [stripped lines]}: from a function's label to its .Lfunc_end (the kernel descriptor lies in between)"""
    out, name, body = {}, None, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            key = name
            for pattern, replacement in renames:
                key = re.sub(pattern, replacement, key)
            out[key], name = body, None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].replace(name, "@")).strip()
        if line:
            body.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPLACEMENT"))
    args = ap.parse_args()
    fa, fb = functions(args.a, args.rename), functions(args.b, args.rename)
    for side, only in ((args.a, sorted(set(fa) - set(fb))), (args.b, sorted(set(fb) - set(fa)))):
        for name in only:
            print(f"only in {side}: {name}")
    common = sorted(set(fa) & set(fb))
    differing = 0
    for name in common:
        if fa[name] != fb[name]:
            differing += 1
            delta = [d for d in difflib.unified_diff(fa[name], fb[name], n=0, lineterm="") if d[0] in "+-" and d[:3] not in ("+++", "---")]
            print(f"differs: {name}: {len(fa[name])} / {len(fb[name])} lines, {sum(d[0] == '-' for d in delta)} / {sum(d[0] == '+' for d in delta)} of them without a partner")
    print(f"{len(fa)} / {len(fb)} functions, {len(common)} in both, {len(common) - differing} identical, {differing} differ")


if __name__ == "__main__":
    main()
