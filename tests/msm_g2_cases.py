"""Shared by tests/test_gpu_msm_g2.py and tests/test_msm_g2_emul.py: the expected
value of a G2 multi-scalar multiplication from the oracle alone (O.g2_mul of every
term, a halving tree of O.g2_add, O.g2_normalize; a zero sum is the (0, one, 0)
image) and the planted edge cases."""
import numpy as np

from oracle import oracle as O

R = O.R
NT = 16


def zero():
    z = np.zeros(24, np.uint64)
    z[8:12] = O.canon_to_mont_array([1]).reshape(4)  # (0, one, 0), one = (1, 0)
    return z


def fr(vals):
    return O.canon_to_mont_array([v % R for v in vals], O.FR).reshape(len(vals), 4)


def g2_points(n, seed):
    """The G2 half of O.random_pairs(n, seed) -- the same scalars times G2::one(), the
    same Jacobian images (z != one) -- without computing its G1 half."""
    _, t = O.random_scalars(n, seed ^ 0x5DEECE66D)
    return O.g2_mul(O.g2_one(), t, NT)


def tree(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 24).copy()
    while a.shape[0] > 1:
        h = (a.shape[0] + 1) // 2
        m = a.shape[0] - h
        a[:m] = O.g2_add(a[:m], a[h:])
        a = a[:h]
    return a


def expect_from_products(prod):
    if prod.shape[0] == 0:
        return zero()
    r = O.g2_normalize(tree(prod))[0]
    return zero() if not r[16:24].any() else r


def expect(p, k):
    p, k = p.reshape(-1, 24), k.reshape(-1, 4)
    return expect_from_products(O.g2_mul(p, k, nthreads=NT) if p.shape[0] else p)


def plant(p, k, positions):
    """Copies of the n points p and Montgomery scalars k with the edge cases planted.
    positions(nw) gives the windows w whose digit boundaries 2^(cw), 2^(cw) - 1,
    2^(cw-1), 2^(cw-1) + 1 are planted for c in {2, 5, 10, 13, 16}."""
    p, k = p.copy(), k.copy()
    n = p.shape[0]
    vals = [None] * n
    p[0] = zero()                              # a zero point with a nonzero scalar
    z2 = p[1].copy()
    z2[16:24] = 0                              # a zero point whose x, y are not zero's
    p[1] = z2
    vals[2] = 0                                # a nonzero point with scalar 0
    p[4], vals[3], vals[4] = p[3], 0x1234567, 0x1234567              # P twice, same scalar: doubling in a bucket
    p[6], vals[5], vals[6] = O.g2_normalize(p[5:6])[0], 99991, 99991   # P in two Jacobian scalings
    p[8], vals[7], vals[8] = O.g2_neg(p[7:8])[0], 31337, 31337        # P and -P: a bucket that cancels
    p[10] = O.g2_normalize(O.g2_neg(p[9:10]))[0]                      # -P in another scaling
    vals[9] = vals[10] = (1 << 200) + 12345
    edge = [1, R - 1, 1 << 253, R - 2, 2]
    for c in (2, 5, 10, 13, 16):
        nw = 254 // c + 1
        for w in positions(nw):
            if c * w < 254:
                edge += [1 << (c * w), (1 << (c * w)) - 1, (1 << (c * w - 1)), (1 << (c * w - 1)) + 1]
    assert 11 + len(edge) <= n, (len(edge), n)
    for j, v in enumerate(edge):
        vals[11 + j] = v
    idx = [j for j, v in enumerate(vals) if v is not None]
    k[idx] = fr([vals[j] for j in idx])
    return p, k
