"""Shared by tests/test_msm_basis_emul.py and tests/test_gpu_msm_basis.py: the expected value of
an MSM over a fixed basis from the oracle alone (O.g1_mul of every term, a halving tree of
O.g1_add, O.g1_normalize; a zero sum is the (0, one, 0) image) and the planted bases and
scalars."""
import numpy as np

from oracle import oracle as O
from tests.msm_prepared_cases import NT, R, fr, g1_points, zero  # noqa: F401


def tree(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 12).copy()
    while a.shape[0] > 1:
        h = (a.shape[0] + 1) // 2
        m = a.shape[0] - h
        a[:m] = O.g1_add(a[:m], a[h:])
        a = a[:h]
    return a


def expect_from_products(prod):
    if prod.shape[0] == 0:
        return zero()
    r = O.g1_normalize(tree(prod))[0]
    return zero() if not r[8:12].any() else r


def expect(p, k):
    p, k = p.reshape(-1, 12), k.reshape(-1, 4)
    return expect_from_products(O.g1_mul(p, k, nthreads=NT) if p.shape[0] else p)


def planted(p, k, c):
    """Copies of the bases p and Montgomery scalars k (at least 24 rows) with the planted rows
    for window width c written over the first ones; the rest stay as they are."""
    p, k = np.array(p, dtype=np.uint64), np.array(k, dtype=np.uint64)
    n = p.shape[0]
    vals = {}
    p[0] = zero()                                   # a zero base, (0, one, 0), with a nonzero scalar
    z2 = p[1].copy()
    z2[8:12] = 0                                    # a zero base under a real x, y
    p[1] = z2
    vals[2] = 0                                     # a nonzero base with scalar 0
    p[4], vals[3], vals[4] = p[3], 0x1234567, 0x1234567                 # B twice, equal scalars: the doubling shortcut
    p[6], vals[5], vals[6] = O.g1_normalize(p[5:6])[0], 99991, 99991    # B in two Jacobian scalings
    p[8], vals[7], vals[8] = O.g1_neg(p[7:8])[0], 31337, 31337          # B and -B: a bucket that cancels
    vals[9], vals[10] = 1, R - 1
    nw = 254 // c + 1
    at = 11
    for w in (1, nw // 2, nw - 1):                  # a low, a middle and the top window
        for v in (1 << (c * w), (1 << (c * w)) - 1):
            if v < 1 << 254:
                vals[at] = v % R
                at += 1
    assert at <= n, (at, n)
    idx = sorted(vals)
    k[idx] = fr([vals[j] for j in idx])
    return p, k
