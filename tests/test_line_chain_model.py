"""The Miller loop's line steps on merged and addend-taking column chains (curve.h
doubling_step / mixed_addition_step with BN_LINE_CHAIN, fq2_split.h "line-step chains"),
modelled on the 9 x 29-bit digits of both lanes with the chains of dot2_asm.inc
interpreted instruction by instruction (test_column_asm.py).

The model composes the two-lane formulas the way the headers do -- own and partner
coordinates, per-lane picks, fq_sub / fq_neg_lazy with their spread K*p, carry passes,
folds, the halving -- and carries every value's static bound code (value <= B p, digits
below L 2^29) as the C++ types do, asserting both after every operation.  Checked:
  - residues: R.x, R.y, R.z and the three coefficients of both steps against the
    reference's formulas (mod.rs:731-776) on Python integers, for random R and base, R
    with z = one, coordinates 0, 1 and p - 1, Fq2 values with one coordinate zero and
    the structured G2 points of edge_vectors;
  - columns: every chain, at the digit bounds of each of its call sites, with all
    operand digits at their admitted maximum (the interpreter asserts < 2^64);
  - value bounds: every chain output within its static bound, with the operand values
    at theirs;
  - the generator: the kinds that existed before come out byte-identical and the
    committed file is what tools/gen_dot2_asm.py emits.
The kernels that run these steps are checked end to end by tests/test_gpu_line_chains.py."""
import hashlib
import importlib.util
import os
import random
import re

import numpy as np
import pytest

from tests import test_column_asm as T

P, R, M29 = T.P, T.R, T.M29
RINV = pow(R, -1, P)
K_MAX_LIMB, K_MAX_BOUND = 7, 160
K_PT = K_LINE = 4
CONSTANTS = os.path.join(T.ROOT, "paritytech-bn_amd", "csrc", "constants.inc")


def const_digits(name):
    m = re.search(r"#define %s \{([^}]*)\}" % name, open(CONSTANTS).read())
    return [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]


def to_digits(x):
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


# ---------------------------------------------------------------- one Fq2 on two lanes
class V:
    """lanes[0] / lanes[1]: the nine digits of coordinate c0 / c1; B, L: the static bound code"""

    def __init__(self, lanes, B, L):
        self.d, self.B, self.L = [list(lanes[0]), list(lanes[1])], B, L
        assert 1 <= B <= K_MAX_BOUND and 1 <= L <= K_MAX_LIMB, (B, L)
        for d in self.d:
            assert all(0 <= v < L << 29 for v in d[:8]) and 0 <= d[8] < 1 << 32, (d, L)
            assert T.value(d) <= B * P, (T.value(d) / P, B)

    def val(self):
        return (T.value(self.d[0]) % P, T.value(self.d[1]) % P)


def sub_spread(L):
    return 0 if L == 1 else L


def kp_spread(K, L):
    r = to_digits(K * P)
    for i in range(8):
        r[i] += (L + 1) << 29
        r[i + 1] -= L + 1
    return r


def lanewise(fn, *vs):
    return [fn(*[v.d[k] for v in vs]) for k in (0, 1)]


def norm(a):
    def f(d):
        d = list(d)
        for i in range(8):
            d[i + 1] += d[i] >> 29
            d[i] &= M29
        return d
    return V(lanewise(f, a), a.B, 1) if a.L > 1 else a


def widen(B, a):
    assert a.B <= B
    return V(a.d, B, a.L)


def add(a, b):
    if a.L + b.L > K_MAX_LIMB:
        return add(norm(a), b) if a.L >= b.L else add(a, norm(b))
    return V(lanewise(lambda x, y: [u + v for u, v in zip(x, y)], a, b), a.B + b.B, a.L + b.L)


def sub(a, b):
    if a.L + sub_spread(b.L) + 2 > K_MAX_LIMB:
        return sub(norm(a), b) if a.L >= b.L else sub(a, norm(b))
    q = kp_spread(b.B + 1, sub_spread(b.L))
    return V(lanewise(lambda x, y: [u + w - v for u, v, w in zip(x, y, q)], a, b), a.B + b.B + 1,
             a.L + sub_spread(b.L) + 2)


def neg_lazy(a):
    q = kp_spread(a.B + 1, sub_spread(a.L))
    return V(lanewise(lambda x: [w - u for u, w in zip(x, q)], a), a.B + 1, sub_spread(a.L) + 2)


def neg(a):
    a = norm(a)
    q = kp_spread(a.B, 0)

    def f(x):  # the top digit is negative until the carry pass (modulo 2^32 on the device)
        t = [w - u for u, w in zip(x, q)]
        for i in range(8):
            t[i + 1] += t[i] >> 29
            t[i] &= M29
        return t
    return V(lanewise(f, a), a.B, 1)


def mul_small(c, a):
    assert c * a.L <= K_MAX_LIMB
    return V(lanewise(lambda x: [u * c for u in x], a), c * a.B, c * a.L)


def half(a):
    a = norm(a)

    def f(x):
        t = [u + (T.P29[i] if x[0] & 1 else 0) for i, u in enumerate(x)]
        for i in range(8):
            t[i + 1] += t[i] >> 29
            t[i] &= M29
        return [(t[i] >> 1) | ((t[i + 1] & 1) << 28) for i in range(8)] + [t[8] >> 1]
    return V(lanewise(f, a), (a.B + 2) // 2, 1)


def fold(a):
    if a.L > 6:
        a = norm(a)

    def f(x):
        q = int(np.float32(x[8]) * np.float32(3.1531629e-07))
        assert q <= a.B
        r, carry = [], 0
        for i in range(8):
            t = x[i] - q * T.P29[i] + carry
            r.append(t & M29)
            carry = t >> 29
        return r + [x[8] - q * T.P29[8] + carry]
    return V(lanewise(f, a), 2, 1)


def narrow(S, a):
    return widen(S, norm(a) if a.B <= S else fold(a))


def partner(a):
    return V([a.d[1], a.d[0]], a.B, a.L)


def pick(a, b):
    """fq_pick(odd, a, b) / fq_select(odd, a, b): the odd lane takes a, the even lane b"""
    return V([b.d[0], a.d[1]], max(a.B, b.B), max(a.L, b.L))


def bcast_c0(a):
    return V([a.d[0], a.d[0]], a.B, a.L)


def split_w(own, ng):
    """dpp_sel_own_partner: the odd lane its own, the even lane the partner's `ng`"""
    return V([ng.d[1], own.d[1]], max(own.B, ng.B), max(own.L, ng.L))


# ---------------------------------------------------------------- the chains
SITES = set()  # (kind, ((B, L) per product operand), ((K, B, L) per addend)) of every call


def dot_bound(prods):
    return 1 + (sum(x.B * y.B for x, y in prods) * 5908 // 1000000 + 1)


def mul_bound(a, b):
    return 1 + (a * b * 5908 + 999999) // 1000000


def chain(asm, kind, ops, adds=(), bound=None):
    """one chain on both lanes; ops: the product operands in the asm's order"""
    prods = list(zip(ops[0::2], ops[1::2]))
    assert sum(x.L * y.L for x, y in prods) <= 6, "column budget"
    assert sum(k * c.L for k, c in adds) <= 1 << 20
    bo = (bound if bound is not None else dot_bound(prods)) + sum(k * c.B for k, c in adds)
    assert bo <= K_MAX_BOUND
    name = kind + ("A%d" % len(adds) if adds else "")
    SITES.add((name, tuple((v.B, v.L) for v in ops), tuple((k, c.B, c.L) for k, c in adds)))
    lanes = []
    for lane in (0, 1):
        arrs = [v.d[lane] for v in ops] + [c.d[lane] for _, c in adds]
        r = T.run(asm[name], bind(arrs, [k for k, _ in adds]))  # asserts every accumulator value < 2^64
        total = sum(T.value(x.d[lane]) * T.value(y.d[lane]) for x, y in prods)
        total += R * sum(k * T.value(c.d[lane]) for k, c in adds)
        T.check(r, total)
        lanes.append(r)
    return V(lanes, bo, 1)


def bind(arrays, ks):
    ops = T.bind(arrays, len(arrays))
    for t, k in enumerate(ks):
        ops[9 + 9 * len(arrays) + 10 + t] = k
    return ops


# ---------------------------------------------------------------- fq2_split.h
def split_mul_cost(la, lb):
    return la * lb + la * max(lb, sub_spread(lb) + 2)


def fq2_mul_split(asm, a, b):
    if split_mul_cost(a.L, b.L) > 6:
        if split_mul_cost(b.L, a.L) <= 6:
            return fq2_mul_split(asm, b, a)
        return fq2_mul_split(asm, norm(a), b) if a.L >= b.L else fq2_mul_split(asm, a, norm(b))
    return chain(asm, "DOT2", [a, bcast_c0(b), partner(a), split_w(b, neg_lazy(b))])


def pre40(a):
    return a if a.B <= 40 else fold(a)


def fq2_mul(asm, a, b):
    return fq2_mul_split(asm, pre40(a), pre40(b))


def fq2_sqr(asm, a):
    own = norm(pre40(a))
    par = partner(own)
    x = pick(own, sub(own, par))
    y = add(par, pick(par, own))
    return chain(asm, "MUL", [x, y], bound=mul_bound(x.B, y.B))


def fq2_mul_xi(a):
    if a.B > 8:
        a = fold(a)
    own = norm(a)

    def times8(x):  # fq_mul_small<8> of a normalized value: carried at once
        t = [u * 8 for u in x]
        for i in range(8):
            t[i + 1] += t[i] >> 29
            t[i] &= M29
        return t
    own9 = add(V(lanewise(times8, own), 8 * own.B, 1), own)
    par = partner(own)
    return add(own9, pick(par, neg_lazy(par)))


def fq2_sqr_sub_msqr(asm, m, g_in, e_in):
    g, e = norm(g_in), norm(e_in)
    pg, pe = partner(g), partner(e)
    x = pick(g, sub(g, pg))
    y = norm(add(pg, pick(pg, g)))
    z = pick(neg_lazy(e), sub(pe, e))
    w = norm(mul_small(m, add(pe, pick(pe, e))))
    return chain(asm, "DOT2", [x, y, z, w])


def fq2_nsqr_add(asm, a_in, b, c):
    own = norm(a_in)
    par = partner(own)
    x = pick(neg_lazy(own), sub(par, own))
    y = add(par, pick(par, own))
    return chain(asm, "MUL", [x, y], [(1, norm(b)), (1, norm(c))], bound=mul_bound(x.B, y.B))


def split_ops(b, nw=False):
    assert b.L == 1
    w = split_w(b, neg_lazy(b))
    return bcast_c0(b), (norm(w) if nw else w)


def split_ops_neg(b):
    assert b.L == 1
    hb = neg_lazy(b)
    return bcast_c0(hb), split_w(hb, b)


def fq2_mul_negb(asm, a, nb):
    assert a.L == 1
    y, w = split_ops_neg(nb)
    return chain(asm, "DOT2", [a, y, partner(a), w])


def fq2_mul_add(asm, a, b, adds):
    assert a.L == 1
    y, w = split_ops(b)
    return chain(asm, "DOT2", [a, y, partner(a), w], adds)


def fq2_dot_pp(asm, a, b, c, d):
    assert a.L == 1 and c.L == 1
    (yb, wb), (yd, wd) = split_ops(b), split_ops(d)
    return chain(asm, "DOT4", [a, yb, partner(a), wb, c, yd, partner(c), wd])


def fq2_dot_pm(asm, a, b, c, d):
    assert a.L == 1 and c.L == 1
    (yb, wb), (yd, wd) = split_ops(b, True), split_ops_neg(d)
    return chain(asm, "DOT4", [a, yb, partner(a), wb, c, yd, partner(c), wd])


# ---------------------------------------------------------------- curve.h, BN_LINE_CHAIN = 3
def g2_coeff_3b():
    def times3(d):
        r, c = [], 0
        for i in range(9):
            t = d[i] * 3 + c
            r.append(t & M29 if i < 8 else t)
            c = t >> 29
        return r
    return V([times3(const_digits("BN_G2B_C0")), times3(const_digits("BN_G2B_C1"))], 3, 1)


def doubling_step(asm, s):
    x, y, z = s
    xy = fq2_mul(asm, x, y)
    b = fq2_sqr(asm, y)
    c = fq2_sqr(asm, z)
    e = fq2_mul(asm, g2_coeff_3b(), c)
    f = add(add(e, e), e)
    g = half(add(b, f))
    nh = fq2_nsqr_add(asm, add(y, z), b, c)
    i = sub(e, b)
    j = fq2_sqr(asm, x)
    sx = narrow(K_PT, fq2_mul(asm, xy, sub(b, g)))
    sy = narrow(K_PT, fq2_sqr_sub_msqr(asm, 3, g, e))
    sz = narrow(K_PT, fq2_mul_negb(asm, norm(b), nh))
    ell = (narrow(K_LINE, fq2_mul_xi(i)), narrow(K_LINE, nh), narrow(K_LINE, add(add(j, j), j)))
    return (sx, sy, sz), ell


def g2_base(q):
    return (neg(q[0]), q[1], neg(q[1]))


def mixed_addition_step(asm, s, base):
    x, y, z = s
    nbx, by, nby = base
    d = narrow(K_LINE, fq2_mul_add(asm, z, nbx, [(1, x)]))
    ne = narrow(K_LINE, fq2_mul_add(asm, z, by, [(1, neg_lazy(y))]))
    f = fq2_sqr(asm, d)
    g = fq2_sqr(asm, ne)
    h = fq2_mul(asm, d, f)
    i = fq2_mul(asm, x, f)
    j = fq2_mul_add(asm, z, g, [(1, h), (2, neg_lazy(i))])
    nx = fq2_mul(asm, d, j)
    ny = fq2_dot_pm(asm, ne, norm(sub(j, i)), h, y)
    nz = fq2_mul(asm, z, h)
    l0 = fq2_mul_xi(fq2_dot_pp(asm, ne, nbx, d, nby))
    return (narrow(K_PT, nx), narrow(K_PT, ny), narrow(K_PT, nz)), (narrow(K_LINE, l0), d, ne)


# ---------------------------------------------------------------- the reference on integers
# values are Montgomery images (x * 2^261 mod p): a product takes one factor 2^-261
def r_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) * RINV % P, (a[0] * b[1] + a[1] * b[0]) * RINV % P)


def r_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def r_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def r_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def r_xi(a):
    return ((9 * a[0] - a[1]) % P, (9 * a[1] + a[0]) % P)


TWO_INV = pow(2, -1, P)


def ref_doubling(s):
    """mod.rs:754-776"""
    x, y, z = s
    bp = (T.value(const_digits("BN_G2B_C0")), T.value(const_digits("BN_G2B_C1")))
    a = r_scale(r_mul(x, y), TWO_INV)
    b = r_mul(y, y)
    c = r_mul(z, z)
    d = r_scale(c, 3)
    e = r_mul(bp, d)
    f = r_scale(e, 3)
    g = r_scale(r_add(b, f), TWO_INV)
    yz = r_add(y, z)
    h = r_sub(r_mul(yz, yz), r_add(b, c))
    i = r_sub(e, b)
    j = r_mul(x, x)
    e_sq = r_mul(e, e)
    out = (r_mul(a, r_sub(b, f)), r_sub(r_mul(g, g), r_scale(e_sq, 3)), r_mul(b, h))
    return out, (r_xi(i), r_sub((0, 0), h), r_scale(j, 3))


def ref_addition(s, base):
    """mod.rs:731-752"""
    x, y, z = s
    bx, by = base
    d = r_sub(x, r_mul(z, bx))
    e = r_sub(y, r_mul(z, by))
    f = r_mul(d, d)
    g = r_mul(e, e)
    h = r_mul(d, f)
    i = r_mul(x, f)
    j = r_sub(r_add(r_mul(z, g), h), r_add(i, i))
    out = (r_mul(d, j), r_sub(r_mul(e, r_sub(i, j)), r_mul(h, y)), r_mul(z, h))
    return out, (r_xi(r_sub(r_mul(e, bx), r_mul(d, by))), d, r_sub((0, 0), e))


# ---------------------------------------------------------------- inputs
def mont(x):
    return x * R % P


def stored(rng, res, bound):
    """a stored Fq2 with the given residues: normalized digits, value res + k p <= bound p"""
    return V([to_digits(r + rng.randrange(bound) * P) for r in res], bound, 1)


def rand_res(rng):
    return (rng.randrange(P), rng.randrange(P))


def edge_fq2():
    one = mont(1)
    vals = [0, one, P - 1, mont(P - 1), 1]
    return [(a, b) for a in vals for b in vals]


def input_sets():
    """(R residues, base residues) : random, z = one, edge coordinates, one coordinate zero,
    the structured G2 points (affine, as the first step sees them, and against a random R)"""
    rng = random.Random(20251)
    sets = [(tuple(rand_res(rng) for _ in range(3)), tuple(rand_res(rng) for _ in range(2))) for _ in range(6)]
    one = (mont(1), 0)
    for _ in range(3):
        q = (rand_res(rng), rand_res(rng))
        sets.append(((q[0], q[1], one), q))
    edges = edge_fq2()
    for k in range(0, len(edges), 3):
        e3 = [edges[(k + t) % len(edges)] for t in range(5)]
        sets.append((tuple(e3[:3]), tuple(e3[3:])))
    for zero_at in (0, 1):
        def hz():
            r = list(rand_res(rng))
            r[zero_at] = 0
            return tuple(r)
        sets.append((tuple(hz() for _ in range(3)), tuple(hz() for _ in range(2))))
    from tests import edge_vectors as E
    for _, qx, qy in E.g2_affine():
        q = (tuple(mont(v) for v in qx), tuple(mont(v) for v in qy))
        sets.append(((q[0], q[1], one), q))
        sets.append((tuple(rand_res(rng) for _ in range(3)), q))
    return sets


@pytest.fixture(scope="module")
def asm():
    m = T.macros()
    assert set(m) >= {"DOT2", "MUL", "DOT2A1", "DOT2A2", "MULA2", "DOT4"}, sorted(m)
    return m


@pytest.fixture(scope="module")
def sets():
    return input_sets()


def same(got, want, what):
    for name, g, w in zip(what, got, want):
        assert g.L == 1 and g.val() == w, name


def test_doubling_step_residues(asm, sets):
    rng = random.Random(1)
    for s_res, _ in sets:
        for bound in (1, K_PT):
            s = tuple(widen(K_PT, stored(rng, r, bound)) for r in s_res)
            (out, ell), (rout, rell) = doubling_step(asm, s), ref_doubling(s_res)
            same(out, rout, ("R.x", "R.y", "R.z"))
            same(ell, rell, ("ell_0", "ell_vw", "ell_vv"))
            assert all(v.B <= K_PT for v in out + ell)


def test_mixed_addition_step_residues(asm, sets):
    rng = random.Random(2)
    for s_res, b_res in sets:
        for bb in (2, K_PT):  # the loop's base (to_affine leaves <= 2 p) and mul_by_q's (kPt)
            s = tuple(widen(K_PT, stored(rng, r, K_PT)) for r in s_res)
            q = tuple(stored(rng, r, bb) for r in b_res)
            for base_res, base in ((b_res, q), ((b_res[0], r_sub((0, 0), b_res[1])), (q[0], neg(q[1])))):
                (out, ell), (rout, rell) = mixed_addition_step(asm, s, g2_base(base)), ref_addition(s_res, base_res)
                same(out, rout, ("R.x", "R.y", "R.z"))
                same(ell, rell, ("ell_0", "ell_vw", "ell_vv"))
                assert all(v.B <= K_PT for v in out + ell)


def test_a_step_chain(asm, sets):
    """doubling, addition, doubling from Q (z = one): each step runs on the model's own
    previous R, as the loop does"""
    rng = random.Random(3)
    for s_res, b_res in sets[6:9]:
        s = tuple(widen(K_PT, stored(rng, r, 1)) for r in s_res)
        q = tuple(stored(rng, r, 2) for r in b_res)
        rs = s_res
        for kind in "dadda":
            if kind == "d":
                (s, ell), (rs, rell) = doubling_step(asm, s), ref_doubling(rs)
            else:
                (s, ell), (rs, rell) = mixed_addition_step(asm, s, g2_base(q)), ref_addition(rs, b_res)
            same(s, rs, ("R.x", "R.y", "R.z"))
            same(ell, rell, ("ell_0", "ell_vw", "ell_vv"))


@pytest.fixture(scope="module")
def sites(asm, sets):
    """the call sites the two steps reach, with their static operand bounds"""
    rng = random.Random(4)
    s_res, b_res = sets[0]
    for bb in (2, K_PT):
        s = tuple(widen(K_PT, stored(rng, r, K_PT)) for r in s_res)
        doubling_step(asm, s)
        mixed_addition_step(asm, s, g2_base(tuple(stored(rng, r, bb) for r in b_res)))
    names = {k for k, _, _ in SITES}
    assert names >= {"DOT2", "MUL", "DOT2A1", "DOT2A2", "MULA2", "DOT4"}, names
    return sorted(SITES)


def at_bound(B, L, digits_max):
    """digits at the digit bound L (all maximal; the top digit within the value bound), or
    the value at the bound B p in normalized digits"""
    if digits_max:
        return [(L << 29) - 1] * 8 + [(B * P) >> 232]
    return to_digits(B * P)


def test_columns_with_maximal_digits(asm, sites):
    """every chain at the digit bounds of each call site, all operand digits maximal: the
    interpreter asserts every accumulator value below 2^64"""
    for name, ops, adds in sites:
        arrs = [at_bound(B, L, True) for B, L in ops] + [at_bound(B, L, True) for _, B, L in adds]
        r = T.run(asm[name], bind(arrs, [k for k, _, _ in adds]))
        assert all(v <= M29 for v in r[:8])


def test_value_bounds_at_operand_bounds(asm, sites):
    """every chain output within its static value bound with the operand values at theirs"""
    for name, ops, adds in sites:
        arrs = [at_bound(B, L, False) for B, L in ops] + [at_bound(B, L, False) for _, B, L in adds]
        r = T.run(asm[name], bind(arrs, [k for k, _, _ in adds]))
        prods = list(zip(ops[0::2], ops[1::2]))
        if name.startswith("MUL"):
            bo = mul_bound(ops[0][0], ops[1][0])
        else:
            bo = 1 + (sum(x[0] * y[0] for x, y in prods) * 5908 // 1000000 + 1)
        bo += sum(k * B for k, B, _ in adds)
        assert bo <= K_MAX_BOUND and T.value(r) <= bo * P, (name, ops, adds, T.value(r) / P, bo)


NEW_KINDS = ("mula1", "mula2", "mula3", "dot4", "dot4a1", "dot4a2")
OLD_KINDS = ("dot2", "mul", "sqr", "dot6", "dot2a1", "dot2a2", "dot2a3", "lin2", "lin3")
# dot2_asm.inc from "// dot2:" to the end, as it stood before the new kinds were appended
OLD_KINDS_SHA256 = "c5817ac3c06cbd91d3649af0eb355d7e5a148025ef92e560a59cd87b9b970dc4"


def test_new_kinds_standalone(asm):
    """the kinds this change adds, over random and maximal digits at the widest budgets the
    wrappers admit: r * 2^261 == sum of products + 2^261 * sum(K_j c_j)  (mod p)"""
    rng = random.Random(6)
    cases = [("MULA%d" % n, (3, 2), n) for n in (1, 2, 3)] + [("MULA2", (6, 1), 2)]
    cases += [("DOT4" + ("A%d" % n if n else ""), b, n) for n in (0, 1, 2)
              for b in ((1, 1, 1, 2, 1, 2, 1, 1), (1, 1, 1, 1, 1, 2, 1, 2), (3, 1, 1, 1, 1, 1, 1, 1))]
    for name, bounds, na in cases:
        for t in range(8):
            arrs = [T.digits(rng, L, t < 2) for L in bounds]
            cs = [T.digits(rng, 7, t in (0, 2))[:8] + [rng.randrange(1 << 20)] for _ in range(na)]
            ks = [(64, 1, 2)[j] for j in range(na)]
            r = T.run(asm[name], bind(arrs + cs, ks))
            total = sum(T.value(x) * T.value(y) for x, y in zip(arrs[0::2], arrs[1::2]))
            T.check(r, total + R * sum(k * T.value(c) for k, c in zip(ks, cs)))


def test_generator_kinds_unchanged_and_current():
    """tools/gen_dot2_asm.py emits the committed file; the kinds that existed before this
    change are byte-identical to a generator without the new kinds (their text does not
    depend on the kinds list) and keep their instruction counts"""
    spec = importlib.util.spec_from_file_location("gen_dot2_asm", os.path.join(T.ROOT, "tools", "gen_dot2_asm.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    m = T.macros()
    assert tuple(g.KINDS) == OLD_KINDS + NEW_KINDS
    assert [k.lower() for k in m] == list(g.KINDS)
    for kind in g.KINDS:
        assert m[kind.upper()] == g.gen(kind), kind
    counts = {"dot2": (287, 243), "mul": (206, 162), "sqr": (170, 126), "dot6": (611, 567), "dot2a1": (296, 252),
              "dot2a2": (305, 261), "dot2a3": (314, 270), "lin2": (35, 18), "lin3": (44, 27)}
    for kind, (n, nmad) in counts.items():
        ins = g.gen(kind)
        assert len(ins) == n and sum(1 for s in ins if s.startswith("v_mad")) == nmad, kind
    # the section of the kinds that existed before, comments included, byte for byte
    text = open(T.INC).read()
    section = text[text.index("// dot2:"):text.index("// mula1:")]
    assert hashlib.sha256(section.encode()).hexdigest() == OLD_KINDS_SHA256
    # the macro bodies of the whole file are the generator's output
    lines = []
    for kind in g.KINDS:
        ins = g.gen(kind)
        lines.append("#define BN_ASM_%s \\" % kind.upper())
        lines += ['    "%s\\n\\t" \\' % s for s in ins[:-1]]
        lines.append('    "%s\\n\\t"' % ins[-1])
    body = [ln for ln in text.split("\n") if ln and not ln.startswith("//") and ln != "#pragma once"]
    assert body == lines
