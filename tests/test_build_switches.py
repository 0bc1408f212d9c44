"""The compile-time switches of the kernel sources and DESIGN.md's table of them
(section 10a) name the same set: a new `#if BN_X` needs a row saying who builds its
other value, and a row whose switch has gone needs deleting."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "paritytech-bn_amd", "csrc")
DESIGN = os.path.join(ROOT, "DESIGN.md")
HEADING = "## 10a. Compile-time switches"


def switches_in_sources():
    """every BN_* name in a #if / #ifdef / #ifndef / #elif line of csrc/*.h and csrc/*.hip
    (dot2_asm.inc is neither; the C header's include guard BN254MI_H does not match BN_)"""
    names = set()
    for path in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")):
        for line in open(path):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                names.update(re.findall(r"\bBN_[A-Z0-9_]+\b", line))
    return names


def switches_in_table():
    """the first cell of every row of the table under HEADING"""
    txt = open(DESIGN).read()
    assert HEADING in txt, "DESIGN.md has no section '%s'" % HEADING
    section = txt.split(HEADING, 1)[1]
    section = re.split(r"^## ", section, maxsplit=1, flags=re.M)[0]
    rows = re.findall(r"^\| `(BN_[A-Z0-9_]+)` \|", section, flags=re.M)
    assert len(rows) == len(set(rows)), "a switch has two rows"
    return set(rows)


def test_design_table_lists_exactly_the_switches_the_sources_test():
    src, doc = switches_in_sources(), switches_in_table()
    assert src, "no switches found: the scan is broken"
    assert src == doc, "in the sources only: %s; in DESIGN.md only: %s" % (sorted(src - doc), sorted(doc - src))
