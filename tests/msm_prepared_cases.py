"""Shared by tests/test_msm_fixed_emul.py and tests/test_gpu_msm_prepared.py: the expected
rows of MSMs over shared bases from the oracle alone (O.g1_mul of every term, a halving
tree of O.g1_add, O.g1_normalize; a zero sum is the (0, one, 0) image) and the planted
bases and scalar rows."""
import numpy as np

from oracle import oracle as O

R = O.R
NT = 16


def zero():
    z = np.zeros(12, np.uint64)
    z[4:8] = O.canon_to_mont_array([1]).reshape(4)  # (0, one, 0)
    return z


def fr(vals):
    return O.canon_to_mont_array([v % R for v in vals], O.FR).reshape(len(vals), 4)


def g1_points(n, seed):
    """s_i * G1::one() for random s_i: Jacobian images with z != one."""
    _, s = O.random_scalars(n, seed)
    return O.g1_mul(O.g1_one(), s, NT)


def products(bases, scalars):
    """(m, k, 12): bases[b] * scalars[j, b].  bases (k, 12), scalars (m, k, 4) Montgomery."""
    k = bases.shape[0]
    m = scalars.shape[0]
    if m == 0:
        return np.zeros((0, k, 12), np.uint64)
    p = np.ascontiguousarray(np.broadcast_to(bases, (m, k, 12))).reshape(-1, 12)
    return O.g1_mul(p, np.ascontiguousarray(scalars).reshape(-1, 4), nthreads=NT).reshape(m, k, 12)


def expect_from_products(prod):
    """(m, 12) expected rows from the (m, k, 12) products: per row a halving tree (odd tail
    carried) of O.g1_add over its k terms, normalized; zero sums as (0, one, 0)."""
    a = np.array(prod, dtype=np.uint64)
    m, k = a.shape[0], a.shape[1]
    if m == 0:
        return np.zeros((0, 12), np.uint64)
    while k > 1:
        h = (k + 1) // 2
        n = k - h
        a[:, :n] = O.g1_add(np.ascontiguousarray(a[:, :n]).reshape(-1, 12),
                            np.ascontiguousarray(a[:, h:k]).reshape(-1, 12)).reshape(m, n, 12)
        k = h
    out = O.g1_normalize(np.ascontiguousarray(a[:, 0]))
    out[~out[:, 8:12].any(axis=1)] = zero()
    return out


def expect(bases, scalars):
    return expect_from_products(products(bases, scalars))


def planted_bases(pts, zero_form):
    """Five bases from the five nonzero points pts: A, A again in another Jacobian scaling,
    B, -B and a zero base -- (0, one, 0) for zero_form 0, z = 0 with foreign x, y for 1."""
    z = zero()
    if zero_form:
        z = pts[4].copy()
        z[8:12] = 0
    return np.stack([pts[0], O.g1_normalize(pts[0:1])[0], pts[2], O.g1_neg(pts[2:3])[0], z])


def planted_values(c):
    """Rows of five canonical scalars for planted_bases at window width c."""
    nw = 254 // c + 1
    s = 0x1f2e3d4c5b6a79880123456789abcdef
    rows = [[0, 0, 0, 0, 0],          # the zero image
            [1, 1, 0, 0, 0],          # A + A: the doubling shortcut
            [0, 0, s, s, 0],          # B and -B: cancels to the zero image
            [0, 0, 1, 1, 0],
            [0, 0, 0, 0, s],          # the zero base alone
            [1, 0, 0, 0, 7],
            [R - 1, 0, 0, 0, 0],
            [R - 1, R - 1, R - 1, R - 2, R - 1],
            [s, R - s, 5, 0, 1]]      # A * s + A * (-s): cancels across two bases, 5 B left
    for w in sorted({1, nw // 2, nw - 1}):
        if w < 1:
            continue
        for v in (1 << (c * w), (1 << (c * w)) - 1, 1 << (c * w - 1), (1 << (c * w - 1)) + 1):
            if v < 1 << 254:
                rows.append([v % R, 3, (v + 1) % R, 0, v % R])
                rows.append([0, v % R, 0, v % R, 2])
    return rows


def planted_scalars(c, m, seed):
    """(m, 5, 4) Montgomery scalars: the planted rows for width c, then random rows."""
    rows = planted_values(c)
    assert len(rows) <= m, (len(rows), m)
    _, k = O.random_scalars((m - len(rows)) * 5, seed=seed, lo=0)
    return np.concatenate([fr([v for row in rows for v in row]).reshape(-1, 5, 4), k.reshape(-1, 5, 4)])
