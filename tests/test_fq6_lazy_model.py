"""The split-layout Fq6 product on six-product column sums (tower.h fq6_mul_uv /
fq_dot6, BN_FQ6_LAZY), modelled on the 9 x 29-bit digits with the chains of
dot2_asm.inc interpreted instruction by instruction (test_column_asm.py).

With xi moved onto the a side,
    c0 = a0 b0 + (xi a1) b2 + (xi a2) b1
    c1 = a0 b1 +     a1  b0 + (xi a2) b2
    c2 = a0 b2 +     a1  b1 +     a2  b0,
each lane sums its coordinate of the three Fq2 products -- own(u) * y + partner(u) * w
with y = v0 and w = (lane 0: K*p - v1, lane 1: v1) -- in one DOT6 chain.  xi * u is
one LIN2 chain, 9 * own + (lane 0: K*p - u1, lane 1: u0).  The model builds every
operand the way the C++ does (fq_neg_lazy's spread K*p, the carry pass of line_ops_of)
and checks, for the operand bounds of every call site (the Fq12 product's a0 b0 and
(a0 + a1)(b0 + b1), the square's a1 a0 and (a0 + a1)(v a1 + a0), and the sparse line
product's contract):
  - the residues against plain arithmetic modulo p;
  - that no accumulator value exceeds 2^64 - 1 (asserted by the interpreter), with
    every digit at 2^29 - 1;
  - that every reduction stays within the value bound fq_dot6 states for it, with
    the operand values at their bounds (2p, 4p, 5p, ...).
The kernels that run these chains are checked end to end by tests/test_gpu_fq6_lazy.py."""
import importlib.util
import os
import random

import pytest

from tests import test_column_asm as T

P, R, M29 = T.P, T.R, T.M29


@pytest.fixture(scope="module")
def asm():
    m = T.macros()
    assert set(m) >= {"DOT6", "LIN2"}, sorted(m)
    return m


def to_digits(x):
    """normalized digits of 0 <= x < 2^261 + slack: the top digit takes what is left"""
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def norm(d):
    """fq_norm: the carry pass over digits 0..7"""
    d = list(d)
    for i in range(8):
        d[i + 1] += d[i] >> 29
        d[i] &= M29
    assert all(0 <= v < (1 << 32) for v in d)
    return d


def neg_lazy(d, bound):
    """fq_neg_lazy of a normalized value <= bound * p: (bound + 1) * p with digits 0..7
    raised by 2^29 (kp_spread(bound + 1, 0)) minus the digits, no carry pass"""
    q = to_digits((bound + 1) * P)
    for i in range(8):
        q[i] += 1 << 29
        q[i + 1] -= 1
    r = [a - b for a, b in zip(q, d)]
    assert all(0 <= v < (2 << 29) for v in r)
    return r


def line_ops(v, bound):
    """line_ops_of: per lane (y, w), normalized; w's value <= (bound + 1) p"""
    v0, v1 = v
    return [(v0, norm(neg_lazy(v1, bound))), (v0, v1)]


def xi_lin(asm, u, bound):
    """fq_xi_lin on both lanes through the LIN2 chain, multipliers (9, 1)"""
    out = []
    for own, other in ((u[0], neg_lazy(u[1], bound)), (u[1], u[0])):
        ops = {9 + i: own[i] for i in range(9)}
        ops.update({18 + i: other[i] for i in range(9)})
        ops[27], ops[28] = 9, 1
        r = T.run(asm["LIN2"], ops)
        assert all(x <= M29 for x in r[:8]) and T.value(r) <= (10 * bound + 1) * P
        out.append(r)
    return out


def dot6(asm, lane, terms):
    """fq_dot6p on one lane: terms = three (u, line_ops) with u = (c0, c1) digit vectors"""
    arrs = []
    for u, v in terms:
        y, w = v[lane]
        arrs += [u[lane], y, u[1 - lane], w]
    return T.run(asm["DOT6"], T.bind(arrs, 12))  # asserts every accumulator value < 2^64


def bound_out(terms_bounds):
    """fq_dot6p's static value bound: BO = 1 + floor(S * 5908 / 10^6) + 1"""
    s = sum(u * (y + y + 1) for u, y in terms_bounds)
    return 1 + (s * 5908 // 1000000 + 1)


def fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def fq2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def fq2_xi(a):
    return ((9 * a[0] - a[1]) % P, (9 * a[1] + a[0]) % P)


def fq6_mul_ref(a, b):
    """fq6.rs:197-207 as the schoolbook sum modulo v^3 = xi"""
    c = [(0, 0)] * 3
    for i in range(3):
        for j in range(3):
            t = fq2_mul(a[i], b[j])
            if i + j >= 3:
                t = fq2_xi(t)
            c[(i + j) % 3] = fq2_add(c[(i + j) % 3], t)
    return c


def fq6_mul_model(asm, a, b, ub, vb):
    """a, b: three Fq2 each as (c0 digits, c1 digits), normalized; ub: the a side's value
    bound, vb: the b side's three.  Returns the three outputs per lane and their bounds."""
    g = ub * 10 + 1
    v = [line_ops(b[k], vb[k]) for k in range(3)]
    g1, g2 = xi_lin(asm, a[1], ub), xi_lin(asm, a[2], ub)
    plan = [  # fq6_mul_uv: (u, its bound, b index) per term, outputs c0, c1, c2
        [(a[0], ub, 0), (g1, g, 2), (g2, g, 1)],
        [(a[0], ub, 1), (a[1], ub, 0), (g2, g, 2)],
        [(a[0], ub, 2), (a[1], ub, 1), (a[2], ub, 0)],
    ]
    out, bounds = [], []
    for row in plan:
        terms = [(u, v[k]) for u, _, k in row]
        out.append([dot6(asm, lane, terms) for lane in (0, 1)])
        bounds.append(bound_out([(bu, vb[k]) for _, bu, k in row]))
    return out, bounds


def vals(e):
    return [(T.value(c[0]) % P, T.value(c[1]) % P) for c in e]


def check_fq6(asm, a, b, ub, vb):
    out, bounds = fq6_mul_model(asm, a, b, ub, vb)
    want = fq6_mul_ref(vals(a), vals(b))
    for k in range(3):
        for lane in (0, 1):
            r = out[k][lane]
            assert all(x <= M29 for x in r[:8])
            assert (T.value(r) * R - want[k][lane]) % P == 0, (k, lane)
            assert T.value(r) <= bounds[k] * P, (k, lane, T.value(r) / P, bounds[k])
    return bounds


def rand_fq2(rng, bound):
    return tuple(to_digits(rng.randrange(bound * P + 1)) for _ in range(2))


# (a side's bound, b side's three bounds) per call site
SITES = {
    "mul aa/bb, sqr ab": (2, (2, 2, 2)),
    "mul (a0+a1)(b0+b1)": (4, (4, 4, 4)),
    "sqr (a0+a1)(v a1 + a0)": (4, (23, 4, 4)),  # xi a1.c2 + a0.c0: 21 + 2
}


@pytest.mark.parametrize("site", sorted(SITES))
def test_residues_random(asm, site):
    ub, vb = SITES[site]
    rng = random.Random(len(site))
    for _ in range(12):
        a = [rand_fq2(rng, ub) for _ in range(3)]
        b = [rand_fq2(rng, vb[k]) for k in range(3)]
        check_fq6(asm, a, b, ub, vb)


@pytest.mark.parametrize("site", sorted(SITES))
def test_values_at_the_bounds(asm, site):
    """every operand at its value bound (u = U p, v0 = Y p, and v1 = 0 so that lane 0's
    w is (Y + 1) p: with Y = 4 the values 2p / 4p, 4p and 5p) and at zero: the reductions
    stay within fq_dot6's stated bound, which is what the callers' folds rely on"""
    ub, vb = SITES[site]
    for a_top in (True, False):
        for b1_zero in (True, False):
            a = [tuple(to_digits(ub * P if a_top else 0) for _ in range(2)) for _ in range(3)]
            b = [(to_digits(vb[k] * P), to_digits(0 if b1_zero else vb[k] * P)) for k in range(3)]
            bounds = check_fq6(asm, a, b, ub, vb)
            assert max(bounds) <= 7  # what tower.h's comment in fq12_mul states


def test_line_product_contract(asm):
    """the sparse line product's call of the shared chain: u <= 2p, y <= 4p, w <= 5p gives
    S = 54 and a reduction below 1.4 p (bound 2)"""
    assert bound_out([(2, 4)] * 3) == 2
    u = (to_digits(2 * P), to_digits(2 * P))
    v = line_ops((to_digits(4 * P), to_digits(0)), 4)
    assert T.value(v[0][1]) == 5 * P
    for lane in (0, 1):
        r = dot6(asm, lane, [(u, v)] * 3)
        assert T.value(r) * 10 <= 14 * P


def test_columns_with_maximal_digits(asm):
    """all twelve operands with every digit at 2^29 - 1 (the digit contract, whatever the
    values): the interpreter asserts each accumulator value below 2^64; so does the LIN2
    chain with a maximal own and the widest fq_neg_lazy digits"""
    top = [M29] * 9
    r = T.run(asm["DOT6"], T.bind([top] * 12, 12))
    T.check(r, 6 * T.value(top) ** 2)
    ops = {9 + i: M29 for i in range(9)}
    ops.update({18 + i: (2 << 29) - 1 for i in range(9)})
    ops[18 + 8] = M29 >> 4  # the value stays below 2^261 (the static bound's job)
    ops[9 + 8] = M29 >> 4
    ops[27], ops[28] = 9, 1
    r = T.run(asm["LIN2"], ops)
    assert all(x <= M29 for x in r[:8])


def test_neg_lazy_and_line_ops_values():
    """the operand forms carry the values the formula needs: w = (Y + 1) p - v1 on lane 0"""
    rng = random.Random(5)
    for bound in (2, 4, 23):
        for _ in range(8):
            v = rand_fq2(rng, bound)
            (y0, w0), (y1, w1) = line_ops(v, bound)
            assert y0 == v[0] and y1 == v[0] and w1 == v[1]
            assert T.value(w0) == (bound + 1) * P - T.value(v[1]) and all(x <= M29 for x in w0[:8])


def test_generator_is_current_fq6():
    """dot2_asm.inc holds what tools/gen_dot2_asm.py writes now for the kinds this product runs"""
    spec = importlib.util.spec_from_file_location("gen_dot2_asm", os.path.join(T.ROOT, "tools", "gen_dot2_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    m = T.macros()
    for kind in ("dot6", "lin2"):
        assert kind in g.KINDS and m[kind.upper()] == g.gen(kind), kind
