#!/usr/bin/env python3
"""Per-kernel comparison of two hipcc -S listings of the same translation unit: for every
kernel of the first listing, the instruction and VALU counts in both and whether the
instruction streams are the same once the numbers the assembler gives its local labels
(.LBBn_m, .Lpost_getpcN: they shift when a kernel is added in front) are taken out.
Shows that a change left the kernels it was not meant to touch as they were.

    python tools/isa_compare.py before.s after.s [SUBSTRING_OF_SYMBOL ...]

With symbol substrings, also prints the opcodes whose counts differ for those kernels."""
import collections
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            t = re.sub(r"\s*;.*$", "", line.strip())
            if t and not t.startswith("."):
                out[cur].append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", t)))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    for k in list(a) + [k for k in b if k not in a]:
        ia, ib = a.get(k, []), b.get(k, [])
        va, vb = (sum(1 for x in i if x.startswith("v_")) for i in (ia, ib))
        what = "same instructions" if ia == ib else "only in one listing" if not ia or not ib else "differs"
        print("%-72s insts %6d -> %6d   VALU %6d -> %6d   %s" % (k[:72], len(ia), len(ib), va, vb, what))
        if ia and ib and ia != ib and any(s in k for s in sys.argv[3:]):
            d = collections.Counter(x.split()[0] for x in ib)
            d.subtract(collections.Counter(x.split()[0] for x in ia))
            print("    opcode counts that changed:", {o: n for o, n in sorted(d.items()) if n})


if __name__ == "__main__":
    main()
