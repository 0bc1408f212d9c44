"""Shared by tests/test_msm_many_emul.py and tests/test_gpu_msm_many.py: the expected rows
of segmented MSMs over fresh bases from the oracle alone (O.g1_mul of every term, a halving
tree of O.g1_add per segment, O.g1_normalize; a zero sum and an empty segment are the
(0, one, 0) image, written out) and the planted segments."""
import numpy as np

from oracle import oracle as O
from tests import msm_prepared_cases as C

R = O.R
NT = 16
zero = C.zero
fr = C.fr
g1_points = C.g1_points


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.uintp)


def products(points, scalars):
    """(n, 12): points[i] * scalars[i].  points (n, 12), scalars (n, 4) Montgomery."""
    if points.shape[0] == 0:
        return np.zeros((0, 12), np.uint64)
    return O.g1_mul(np.ascontiguousarray(points), np.ascontiguousarray(scalars), nthreads=NT)


def expect_from_products(prod, offsets):
    """(m, 12) expected rows from the (n, 12) products: per segment a halving tree (odd tail
    carried) of O.g1_add, normalized; zero sums and empty segments as (0, one, 0).  One
    O.g1_add call per level over all segments."""
    off = [int(x) for x in offsets]
    m = len(off) - 1
    if m == 0:
        return np.zeros((0, 12), np.uint64)
    cur = [np.array(prod[off[j]:off[j + 1]], dtype=np.uint64).reshape(-1, 12) for j in range(m)]
    while any(len(s) > 1 for s in cur):
        a, b, where = [], [], []
        for j, s in enumerate(cur):
            k = len(s)
            if k > 1:
                h = (k + 1) // 2
                a.append(s[:k - h])
                b.append(s[h:k])
                where.append((j, k - h, h))
        sums = O.g1_add(np.ascontiguousarray(np.concatenate(a)), np.ascontiguousarray(np.concatenate(b)))
        pos = 0
        for j, n, h in where:
            cur[j] = np.concatenate([sums[pos:pos + n], cur[j][n:h]])
            pos += n
    rows = np.stack([s[0] if len(s) else zero() for s in cur])
    out = O.g1_normalize(np.ascontiguousarray(rows))
    out[~out[:, 8:12].any(axis=1)] = zero()
    return out


def expect(points, scalars, offsets):
    return expect_from_products(products(points, scalars), offsets)


def planted(pts, c, zero_form):
    """Segments of five terms over C.planted_bases (A, A in another Jacobian scaling, B, -B,
    a zero point in the given form) with the scalar rows of C.planted_values(c): scalars 0, 1
    and r - 1, the digit-boundary values, equal terms and P with -P side by side (in one unit
    for every T >= 2), sums that cancel to zero.  Returns (points, canonical scalars, offsets)."""
    rows = C.planted_values(c)
    bases = C.planted_bases(pts, zero_form)
    points = np.ascontiguousarray(np.tile(bases, (len(rows), 1)))
    vals = [v for row in rows for v in row]
    return points, vals, offsets_of([5] * len(rows))
