#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two sets of `hipcc --cuda-device-only -S` listings: do the same kernels (matched by mangled
name) have the same instruction stream once local label numbers and comments are dropped?  One line per kernel, then the totals.
usage: python tools/isa_compare.py A.s [A2.s ...] -- B.s [B2.s ...]      (exit status 1 if any kernel differs or is missing)"""
import re
import sys


def kernels(paths):
    """mangled kernel name -> normalised instruction lines, over all listings of one side"""
    out = {}
    for path in paths:
        lines = open(path).read().split("\n")
        names = {m.group(1) for l in lines if (m := re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", l))}
        cur = None
        for l in lines:
            m = re.match(r"^(\S+):", l)
            if cur is None and m and m.group(1) in names:
                cur = m.group(1)
                assert cur not in out, f"{cur} is defined in two listings"
                out[cur] = []
            elif cur is not None and re.match(r"^\.Lfunc_end\d+:", l):
                cur = None
            elif cur is not None:
                l = l.split(";")[0].strip()
                if l and not l.startswith("."):          # instructions only: no labels, no directives
                    out[cur].append(re.sub(r"\.L\w*?\d+(_\d+)?", lambda k: ".L" + (k.group(1) or ""), l))
    return out


def main():
    args = sys.argv[1:]
    if "--" not in args:
        sys.exit(__doc__)
    a, b = kernels(args[:args.index("--")]), kernels(args[args.index("--") + 1:])
    differ = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "only in " + ("A" if name in a else "B")
        else:
            verdict = "equal" if a[name] == b[name] else f"NOT EQUAL ({len(a[name])} / {len(b[name])} instructions)"
        differ += verdict != "equal"
        print(f"{verdict:12s} {name}")
    print(f"{len(set(a) | set(b))} kernels, {differ} not equal or missing")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
