"""The pairing on scaled inputs (pairing.h scaled_inputs): where only Gt leaves a pairing
the Miller loop runs on (N^2 X_P, N^3 Y_P), (m^2 X_Q, m^3 Y_Q) and the curve constant
l^6 b' -- N = N(Z_Q), l = N Z_P, m = Z_P conj(Z_Q) -- instead of the affine points, and
the final exponentiation removes the power of l in Fq* that the Miller value picks up.

  - the identity on integers: the 87 coefficients built with these formulas in Python Fq2
    arithmetic, through the oracle's miller_loop and final_exponentiation, give the
    oracle's pairing bit for bit;
  - the engine's own code on the host (tests/native/scaled_emul.cpp: scaled_inputs ->
    miller_fused -> fe_first_chunk / fe_last_chunk from the device headers, with the
    fold-bound checks of BN_HOST_CHECKS) gives the same Gt, and one for a zero point;
  - split form: the lane model of tests/test_line_chain_model.py runs doubling_step with
    the constant replaced by an operand at the stated bound (value <= 3 p, normalized
    digits) with maximal digits: columns below 2^64, outputs within their value bounds,
    residues those of the reference's step with the scaled constant.
The kernels are checked end to end by tests/test_gpu_scaled_inputs.py."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E
from tests import test_line_chain_model as M
from tests.native import scaledemul

P = O.P
NAF = [1, 0, 1, 0, 0, 0, 3, 0, 3, 0, 0, 0, 3, 0, 1, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 1, 0, 0, 3, 0, 1, 0,
       0, 3, 0, 0, 0, 0, 3, 0, 1, 0, 0, 0, 3, 0, 3, 0, 0, 1, 0, 0, 0, 3, 0, 0, 3, 0, 1, 0, 1, 0, 0, 0]


# ---------------------------------------------------------------- Fq2 on Python integers
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def f2neg(a):
    return f2sub((0, 0), a)


def f2conj(a):
    return (a[0], -a[1] % P)


def f2inv(a):
    t = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * t % P, -a[1] * t % P)


def f2pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2mul(r, a)
        a = f2mul(a, a)
        e >>= 1
    return r


XI = (9, 1)
B_TWIST = f2mul((3, 0), f2inv(XI))  # b' = 3 / xi (mod.rs:452-467)
TWIST_Q_X = f2pow(XI, (P - 1) // 3)
TWIST_Q_Y = f2pow(XI, (P - 1) // 2)
TWO_INV = pow(2, -1, P)


def doubling(r, b):
    """mod.rs:754-776 with the curve constant b"""
    x, y, z = r
    a = f2scale(f2mul(x, y), TWO_INV)
    bb = f2mul(y, y)
    c = f2mul(z, z)
    e = f2mul(b, f2scale(c, 3))
    f = f2scale(e, 3)
    g = f2scale(f2add(bb, f), TWO_INV)
    yz = f2add(y, z)
    h = f2sub(f2mul(yz, yz), f2add(bb, c))
    i = f2sub(e, bb)
    j = f2mul(x, x)
    e_sq = f2mul(e, e)
    out = (f2mul(a, f2sub(bb, f)), f2sub(f2mul(g, g), f2scale(e_sq, 3)), f2mul(bb, h))
    return out, (f2mul(XI, i), f2neg(h), f2scale(j, 3))


def addition(r, base):
    """mod.rs:731-752"""
    x, y, z = r
    bx, by = base
    d = f2sub(x, f2mul(z, bx))
    e = f2sub(y, f2mul(z, by))
    f = f2mul(d, d)
    g = f2mul(e, e)
    h = f2mul(d, f)
    i = f2mul(x, f)
    j = f2sub(f2add(f2mul(z, g), h), f2add(i, i))
    out = (f2mul(d, j), f2sub(f2mul(e, f2sub(i, j)), f2mul(h, y)), f2mul(z, h))
    return out, (f2mul(XI, f2sub(f2mul(e, bx), f2mul(d, by))), d, f2neg(e))


def mul_by_q(q):
    """mod.rs:694-699"""
    return (f2mul(TWIST_Q_X, f2conj(q[0])), f2mul(TWIST_Q_Y, f2conj(q[1])))


def coefficients(q, b):
    """AffineG2::precompute (mod.rs:701-727) from (x, y) with the curve constant b -> the
    (87, 24) images of (ell_0, ell_vw, ell_vv)"""
    r = (q[0], q[1], (1, 0))
    nq = (q[0], f2neg(q[1]))
    ells = []
    for d in NAF:
        r, ell = doubling(r, b)
        ells.append(ell)
        if d:
            r, ell = addition(r, q if d == 1 else nq)
            ells.append(ell)
    q1 = mul_by_q(q)
    q2 = mul_by_q(q1)
    q2 = (q2[0], f2neg(q2[1]))
    r, ell = addition(r, q1)
    ells.append(ell)
    r, ell = addition(r, q2)
    ells.append(ell)
    assert len(ells) == 87
    return O.canon_to_mont_array([v for ell in ells for c in ell for v in c]).reshape(87, 24)


def scaled(p_row, q_row):
    """the scaled coordinates and constant of one Jacobian pair, on integers"""
    xp, yp, zp = O.mont_array_to_canon(p_row)
    c = O.mont_array_to_canon(q_row)
    xq, yq, zq = (c[0], c[1]), (c[2], c[3]), (c[4], c[5])
    n = (zq[0] * zq[0] + zq[1] * zq[1]) % P
    lam = n * zp % P
    m = f2scale(f2conj(zq), zp)
    m2 = f2mul(m, m)
    px, py = n * n * xp % P, n * n * n * yp % P
    q = (f2mul(m2, xq), f2mul(f2mul(m2, m), yq))
    return px, py, q, f2scale(B_TWIST, pow(lam, 6, P))


def gt_from_coefficients(px, py, q, b):
    f = O.miller_loop(coefficients(q, b), O.canon_to_mont_array([px]), O.canon_to_mont_array([py]))
    gt, rcs = O.final_exponentiation(f.reshape(1, 48))
    assert rcs == [0]
    return gt[0]


# ---------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def rows():
    """(p, q, labels, the oracle's Gt): random Jacobian pairs, z = one on one side and on
    both, Z_Q with one coordinate zero, the non-zero structured pairs"""
    p, q, _, _ = O.random_pairs(8, seed=2029, nthreads=8)
    pn, qn = O.g1_normalize(p[:3]), O.g2_normalize(q[:3])
    ps, qs, labels = [p], [q], ["random %d" % i for i in range(8)]
    ps += [pn[:1], p[1:2], pn[2:3]]
    qs += [q[:1], qn[1:2], qn[2:3]]
    labels += ["only P at z = one", "only Q at z = one", "both at z = one"]
    g2 = E.g2_affine()[:2]
    v = 0x1234567 * pow(3, 200, P) % P
    ps.append(p[3:5])
    qs.append(E.g2_jacobian(g2, [(0, v), (v, 0)]))
    labels += ["Z_Q.c0 = 0", "Z_Q.c1 = 0"]
    sp, sq, sl = E.pairing_pairs()
    ps.append(sp)
    qs.append(sq)
    labels += sl
    p, q = np.concatenate(ps), np.concatenate(qs)
    assert not (p[:, 8:] == 0).all(axis=1).any() and not (q[:, 16:] == 0).all(axis=1).any()
    return p, q, labels, O.pairing_many(p, q, 8)


def test_python_formulas_are_the_reference_on_affine_inputs():
    """the model itself: with the true affine point and b' the coefficients are the oracle's"""
    _, q, _, _ = O.random_pairs(2, seed=7, nthreads=2)
    aff, rcs = O.g2_to_affine(q)
    assert rcs == [0, 0]
    for k in range(2):
        c = O.mont_array_to_canon(aff[k])
        assert np.array_equal(coefficients(((c[0], c[1]), (c[2], c[3])), B_TWIST), O.g2_precompute(aff[k]))


def test_identity_on_integers(rows):
    p, q, labels, want = rows
    for k in range(p.shape[0]):
        assert np.array_equal(gt_from_coefficients(*scaled(p[k], q[k])), want[k]), labels[k]


def test_engine_code_on_the_host(rows):
    p, q, labels, want = rows
    for k in range(p.shape[0]):
        got, skip = scaledemul.pairing_scaled(p[k], q[k])
        assert skip == 0 and np.array_equal(got, want[k]), labels[k]


def test_engine_code_zero_points_give_one(rows):
    p, q, _, _ = rows
    one = O.canon_to_mont_array([1] + [0] * 11)
    for pz, qz in ((E.zero_point(12), q[0]), (p[0], E.zero_point(24)), (E.zero_point(12), E.zero_point(24))):
        assert np.array_equal(O.pairing_many(pz.reshape(1, 12), qz.reshape(1, 24))[0], one)
        got, skip = scaledemul.pairing_scaled(pz, qz)
        assert skip == 1 and np.array_equal(got, one)


# ---------------------------------------------------------------- split form: the operand's bounds
def coeff_operands():
    """3 b'' as doubling_step takes it with BN_LINE_CHAIN & 1: value <= 3 p, normalized digits.
    All digits maximal (the top digit one short of 3 p's, so the value stays below 3 p), the
    value at 3 p and next to it, at one, and random values below 3 p."""
    rng = random.Random(77)
    top = (3 * P) >> 232
    maximal = [M.M29] * 8 + [top - 1]
    ops = [[maximal, maximal], [M.to_digits(3 * P), M.to_digits(3 * P - 1)], [M.to_digits(1), maximal]]
    ops += [[M.to_digits(rng.randrange(3 * P + 1)) for _ in (0, 1)] for _ in range(3)]
    return [M.V(lanes, 3, 1) for lanes in ops]


def test_split_doubling_step_with_operand_at_its_bound(monkeypatch):
    asm = M.T.macros()
    rng = random.Random(5)
    three_inv = pow(3, -1, P)
    for op in coeff_operands():
        # the reference's step with b'' = (the operand's residue) / 3 as its constant
        b2 = [v * three_inv % P for v in op.val()]
        digits = {"BN_G2B_C0": M.to_digits(b2[0]), "BN_G2B_C1": M.to_digits(b2[1])}
        monkeypatch.setattr(M, "g2_coeff_3b", lambda op=op: op)
        monkeypatch.setattr(M, "const_digits", lambda name, digits=digits: digits[name])
        for s_res, _ in M.input_sets():
            for bound in (1, M.K_PT):
                s = tuple(M.widen(M.K_PT, M.stored(rng, r, bound)) for r in s_res)
                # (every chain asserts its columns below 2^64, every value its static bounds)
                (out, ell), (rout, rell) = M.doubling_step(asm, s), M.ref_doubling(s_res)
                M.same(out, rout, ("R.x", "R.y", "R.z"))
                M.same(ell, rell, ("ell_0", "ell_vw", "ell_vv"))
                assert all(v.B <= M.K_PT for v in out + ell)
        # R with every digit maximal at its bound against the maximal operand
        top4 = (M.K_PT * P) >> 232
        big = M.V([[M.M29] * 8 + [top4 - 1]] * 2, M.K_PT, 1)
        out, ell = M.doubling_step(asm, (big, big, big))
        rout, rell = M.ref_doubling((big.val(),) * 3)
        M.same(out, rout, ("R.x", "R.y", "R.z"))
        M.same(ell, rell, ("ell_0", "ell_vw", "ell_vv"))
