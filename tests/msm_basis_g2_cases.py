"""Shared by tests/test_msm_basis_g2_emul.py and tests/test_gpu_msm_basis_g2.py: the expected
value of a G2 MSM over a fixed basis from the oracle alone (tests/msm_g2_cases.py: O.g2_mul of
every term, a halving tree of O.g2_add, O.g2_normalize), the planted bases and scalars of
tests/msm_basis_cases.planted restated over G2, and one on-curve base outside the order-r
subgroup."""
import numpy as np

from oracle import oracle as O
from tests.msm_g2_cases import NT, R, expect, expect_from_products, fr, g2_points, tree, zero  # noqa: F401

OFF_AT = 23   # the row of the off-subgroup base: the last of the 24 rows planted() may write


def off_subgroup_point(seed=0x7157):
    """The (x, y, one) image of a point of E'(Fq2) outside the order-r subgroup."""
    from tests import group_exceptional_cases as X
    x, y = X.random_twist_points(1, seed)
    p = np.zeros(24, np.uint64)
    p[0:8], p[8:16] = x[0], y[0]
    p[16:20] = O.canon_to_mont_array([1]).reshape(4)
    return p


def planted(p, k, c):
    """Copies of the bases p and Montgomery scalars k (at least 24 rows) with the planted rows
    for window width c written over the first ones; the rest stay as they are."""
    p, k = np.array(p, dtype=np.uint64), np.array(k, dtype=np.uint64)
    n = p.shape[0]
    vals = {}
    p[0] = zero()                                   # a zero base, (0, one, 0), with a nonzero scalar
    z2 = p[1].copy()
    z2[16:24] = 0                                   # a zero base under a real x, y
    p[1] = z2
    vals[2] = 0                                     # a nonzero base with scalar 0
    p[4], vals[3], vals[4] = p[3], 0x1234567, 0x1234567                 # B twice, equal scalars: the doubling shortcut
    p[6], vals[5], vals[6] = O.g2_normalize(p[5:6])[0], 99991, 99991    # B in two Jacobian scalings
    p[8], vals[7], vals[8] = O.g2_neg(p[7:8])[0], 31337, 31337          # B and -B: a bucket that cancels
    vals[9], vals[10] = 1, R - 1
    nw = 254 // c + 1
    at = 11
    for w in (1, nw // 2, nw - 1):                  # a low, a middle and the top window
        for v in (1 << (c * w), (1 << (c * w)) - 1):
            if v < 1 << 254:
                vals[at] = v % R
                at += 1
    assert at <= OFF_AT < n, (at, n)
    idx = sorted(vals)
    k[idx] = fr([vals[j] for j in idx])
    return p, k
