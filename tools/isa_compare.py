#!/usr/bin/env python3
"""Per-kernel comparison of two hipcc -S listings of the same translation unit: for every
kernel of the first listing, the instruction and VALU counts in both and whether the
instruction streams are the same once the numbers the assembler gives its local labels
(.LBBn_m, .Lpost_getpcN: they shift when a kernel is added in front) are taken out.
Shows that a change left the kernels it was not meant to touch as they were.

    python tools/isa_compare.py [--descriptors] before.s after.s [SUBSTRING_OF_SYMBOL ...]

With symbol substrings, also prints the opcodes whose counts differ for those kernels.
With --descriptors, also compares each kernel's descriptor (the .amdhsa_* lines: VGPRs,
SGPRs, scratch, LDS) and appends "same descriptor" or the lines that differ.  The exit
status is 1 if anything differs or a symbol is in one listing only."""
import collections
import re
import sys


def kernels(path):
    out, cur, funcs = {}, None, set()
    for line in open(path):
        t = re.match(r"^\s*\.type\s+(_Z\w+),@function", line)
        if t:
            funcs.add(t.group(1))
        m = re.match(r"^(_Z\w+):", line)
        if m:  # (a data object's label, e.g. a constant table, ends the function before it)
            cur = m.group(1) if m.group(1) in funcs else None
            if cur:
                out[cur] = []
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            t = re.sub(r"\s*;.*$", "", line.strip())
            if t and not t.startswith("."):
                out[cur].append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", t)))
    return out


def descriptors(path):
    """kernel -> its .amdhsa_* lines (the block between .amdhsa_kernel and .end_amdhsa_kernel)"""
    out, cur = {}, None
    for line in open(path):
        t = line.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = t.split()[1]
            out[cur] = []
        elif t.startswith(".end_amdhsa_kernel"):
            cur = None
        elif cur is not None and t.startswith(".amdhsa_"):
            out[cur].append(re.sub(r"\s+", " ", t))
    return out


def main():
    args = sys.argv[1:]
    desc = "--descriptors" in args
    args = [x for x in args if x != "--descriptors"]
    a, b = kernels(args[0]), kernels(args[1])
    da, db = (descriptors(args[0]), descriptors(args[1])) if desc else ({}, {})
    bad = 0
    for k in list(a) + [k for k in b if k not in a]:
        ia, ib = a.get(k, []), b.get(k, [])
        va, vb = (sum(1 for x in i if x.startswith("v_")) for i in (ia, ib))
        what = "same instructions" if ia == ib else "only in one listing" if not ia or not ib else "differs"
        bad += ia != ib
        if desc and (k in da or k in db):
            same = da.get(k) == db.get(k)
            bad += not same
            what += "   same descriptor" if same else "   DESCRIPTOR DIFFERS: %s" % sorted(
                set(da.get(k, [])) ^ set(db.get(k, [])))
        print("%-72s insts %6d -> %6d   VALU %6d -> %6d   %s" % (k[:72], len(ia), len(ib), va, vb, what))
        if ia and ib and ia != ib and any(s in k for s in args[2:]):
            d = collections.Counter(x.split()[0] for x in ib)
            d.subtract(collections.Counter(x.split()[0] for x in ia))
            print("    opcode counts that changed:", {o: n for o, n in sorted(d.items()) if n})
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
