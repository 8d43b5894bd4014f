#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two sets of `hipcc --cuda-device-only -S` listings: do the same kernels (matched by mangled
name) have the same instruction stream once local label numbers and comments are dropped?  One line per kernel, then the totals.
usage: python tools/isa_compare.py [--existing] A.s [A2.s ...] -- B.s [B2.s ...]      (exit status 1 if any kernel differs or is missing)
--existing: only the kernels of A are judged ("did every kernel that existed keep its stream?"): kernels only in B are listed as new,
and a kernel of A whose name is gone is matched to the kernel of B that is the same template with arguments appended and the same
parameter list -- foo<1, false>(float*) and foo<1, false, float>(float*): a template that gained a defaulted or deduced argument
(needs c++filt)."""
import re
import subprocess
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


def split_demangled(d):
    """'ns::foo<1, false>(float*, int)' -> ('ns::foo', '1, false', '(float*, int)'); no template arguments: ('ns::foo', None, '(...)')"""
    depth = 0
    for i, ch in enumerate(d):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0 and not d.startswith("(anonymous namespace)", i):
            head, params = d[:i], d[i:]
            break
    else:
        return d, None, ""
    if not head.endswith(">"):
        return head, None, params
    depth = 0
    for i in range(len(head) - 1, -1, -1):
        depth += head[i] == ">"
        depth -= head[i] == "<"
        if depth == 0:
            return head[:i], head[i + 1:-1], params
    return head, None, params


def renamed(a, b):
    """kernel of A without a namesake in B -> the kernel of B it became (see --existing), where there is exactly one"""
    gone, fresh = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    if not gone or not fresh:
        return {}
    out = subprocess.run(["c++filt"], input="\n".join(gone + fresh), capture_output=True, text=True, check=True).stdout.split("\n")
    dem = dict(zip(gone + fresh, out))
    found = {}
    for g in gone:
        base, targs, params = split_demangled(dem[g])
        if targs is None:
            continue
        hits = [f for f in fresh if (lambda fb, ft, fp: fb == base and fp == params and ft is not None and ft.startswith(targs + ", "))(
            *split_demangled(dem[f]))]
        if len(hits) == 1:
            found[g] = hits[0]
    return found


def main():
    args = sys.argv[1:]
    existing = "--existing" in args
    if existing:
        args.remove("--existing")
    if "--" not in args:
        sys.exit(__doc__)
    a, b = kernels(args[:args.index("--")]), kernels(args[args.index("--") + 1:])
    differ = 0
    if existing:
        became = renamed(a, b)
        for name in sorted(a):
            other = name if name in b else became.get(name)
            verdict = "missing" if other is None else "equal" if a[name] == b[other] else f"NOT EQUAL ({len(a[name])} / {len(b[other])} instructions)"
            differ += verdict != "equal"
            print(f"{verdict:12s} {name}" + (f"  (now {other})" if other not in (None, name) else ""))
        new = sorted(set(b) - set(a) - set(became.values()))
        for name in new:
            print(f"{'new':12s} {name}")
        print(f"{len(a)} kernels that existed, {differ} not equal or missing; {len(new)} new")
        sys.exit(1 if differ else 0)
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
