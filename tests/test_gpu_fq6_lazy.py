"""The split-layout Fq12 product and square over six-product column sums (tower.h
fq6_mul_uv / fq_dot6, BN_FQ6_LAZY), bit for bit against the oracle.
kernels_pairing.hip builds that form (and the cyclotomic square's linear chains,
BN_CYC_LIN); kernels_fe.hip and kernels_gtpow.hip keep the Karatsuba form (DESIGN.md
4.6).  fq12_op_many therefore runs the step machine's OP_MUL / OP_SQR / OP_CYC twice:
on the default context (kernels_fe.hip's k_fq12_vm, Karatsuba) and on a context with
set_fq12_op_unit(1) (kernels_pairing.hip's k_fq12_vm_pairing: the operations exactly as
k_pairing_full runs them, the column-sum form).  The operand rows put a nonzero value
into every slot of every chain in turn, make the Karatsuba sums a.c0 + a.c1 vanish or
take their largest value, and place the internal 29-bit digits at 0 and 2^29 - 1.
k_pairing_full's Miller squarings and final-exponentiation products (pairing_many on
the throughput path) and k_miller_seg's squarings (pairing_batch) run on random
pairings.  k_gt_pow and final_exponentiation_many are not repeated here: their units
did not change.  tests/test_fq6_lazy_model.py checks the chains' bounds on the CPU.
Runs on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
NT = 16
NROWS = 257
P = O.P
M29 = (1 << 29) - 1
ONE12 = [1] + [0] * 11


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module", params=["fe_unit", "pairing_unit"])
def opctx(request):
    """fq12_op_many on kernels_fe.hip's step machine (the Karatsuba products) and on
    kernels_pairing.hip's (the column-sum products and the linear cyclotomic chains)"""
    from substrate_bn import Context
    c = Context(0)
    if request.param == "pairing_unit":
        c.set_fq12_op_unit(1)
    return c


@pytest.fixture(scope="module")
def ctx_tp():
    """Every pairing_many batch on the throughput path (k_pairing_full, the kernel
    bench.py's headline measures): the latency-path threshold is 0."""
    from substrate_bn import Context
    c = Context(0)
    c.set_fe_wide_max(0)
    return c


def digit_patterns():
    """canonical values whose internal form (x * 2^261 mod p, nine 29-bit digits) has
    its digits at 0 and 2^29 - 1: even digits set, odd digits set, digits 0..7 set under
    the largest top digit that keeps the value below p"""
    even = sum(M29 << (29 * i) for i in range(0, 8, 2))
    odd = sum(M29 << (29 * i) for i in range(1, 8, 2))
    full = even + odd + (((P >> 232) - 1) << 232)
    rinv = pow(1 << 261, -1, P)
    return [m * rinv % P for m in (even, odd, full)]


def build_rows():
    """257 operand pairs (a, b) as lists of twelve canonical coefficients, in the order
    c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (two Fq each); the first two rows are the
    ones a batch of 1 or 2 runs"""
    g = O.SplitMix64(6021)
    rnd = lambda: [g.below(P) for _ in range(12)]  # noqa: E731
    neg6 = lambda x: x[:6] + [(P - v) % P for v in x[:6]]  # noqa: E731  c1 = -c0
    a, b = [], []

    def add(x, y):
        a.append(list(x))
        b.append(list(y))

    add([P - 1] * 12, [P - 1] * 12)               # maximal coefficients and sums
    add(neg6(rnd()), neg6(rnd()))                 # a.c0 + a.c1 == 0 and b.c0 + b.c1 == 0
    small = [0, 1, P - 1, P - 2]
    for x in small:                               # every coefficient one of the four, all pairs
        for y in small:
            add([x] * 12, [y] * 12)
    for x in small:                               # the four mixed within one element
        add([small[(k + small.index(x)) % 4] for k in range(12)], rnd())
    pats = digit_patterns()
    for x in pats:
        for y in pats:
            add([x] * 12, [y] * 12)
        add([x] * 12, rnd())
        add(rnd(), [pats[(k + pats.index(x)) % 3] for k in range(12)])
    for k in range(6):                            # b with one nonzero Fq2 coefficient
        y = [0] * 12
        y[2 * k], y[2 * k + 1] = g.below(P), g.below(P)
        add(rnd(), y)
        y = [0] * 12
        y[2 * k + (k & 1)] = P - 1                # and with one nonzero Fq
        add([P - 1] * 12, y)
    for k in range(6):                            # the same on the a side
        x = [0] * 12
        x[2 * k], x[2 * k + 1] = g.below(P), g.below(P)
        add(x, rnd())
    add(neg6([P - 1] * 12), neg6([1] * 12))
    add(neg6(rnd()), rnd())
    add(rnd(), neg6(rnd()))
    add(rnd(), ONE12)                             # a * 1, a * 0, 1 * b, 0 * b
    add(rnd(), [0] * 12)
    add(ONE12, rnd())
    add([0] * 12, rnd())
    while len(a) < NROWS:
        add(rnd(), rnd())
    assert len(a) == NROWS
    return a, b


@pytest.fixture(scope="module")
def rows():
    """the operand rows as Montgomery images with the oracle's product and square of
    each: computed once, read-only"""
    a, b = build_rows()
    A = O.canon_to_mont_array([v for r in a for v in r]).reshape(NROWS, 48)
    B = O.canon_to_mont_array([v for r in b for v in r]).reshape(NROWS, 48)
    d = {"a": A, "b": B, "mul": O.binary("orc_fq12_mul", A, B, 48, 48, 48),
         "sqr_a": O.unary("orc_fq12_squared", A, 48)[0], "sqr_b": O.unary("orc_fq12_squared", B, 48)[0],
         "cyc_a": O.unary("orc_fq12_cyclotomic_squared", A, 48)[0]}
    for v in d.values():
        v.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def ref():
    """257 random pairs in Jacobian form and the generators, with the oracle's Gt"""
    _, S = O.random_scalars(NROWS, seed=6023, lo=1)
    p = O.g1_mul(np.tile(O.g1_one(), (NROWS, 1)), S, NT)
    q = O.g2_mul(np.tile(O.g2_one(), (NROWS, 1)), np.roll(S, 5, axis=0), NT)
    pa, qa = np.array(O.g1_one()).reshape(1, 12), np.array(O.g2_one()).reshape(1, 24)
    d = {"p": p, "q": q, "gt": O.pairing_many(p, q, NT), "pa": pa, "qa": qa, "gta": O.pairing_many(pa, qa)}
    for v in d.values():
        v.setflags(write=False)
    return d


def same(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%s: rows %s of %d differ" % (what, bad[:8], want.shape[0])


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_op_mul(opctx, rows, n):
    same(opctx.fq12_op_many("mul", rows["a"][:n], rows["b"][:n]), rows["mul"][:n], "mul")


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_op_sqr(opctx, rows, n):
    same(opctx.fq12_op_many("sqr", rows["a"][:n]), rows["sqr_a"][:n], "sqr a")
    same(opctx.fq12_op_many("sqr", rows["b"][:n]), rows["sqr_b"][:n], "sqr b")


def test_op_mul_is_sqr_on_equal_operands(opctx, rows):
    same(opctx.fq12_op_many("mul", rows["a"], rows["a"]), rows["sqr_a"], "a * a")


def test_op_cyc_sqr(opctx, rows):
    """the Granger-Scott formula is defined for any Fq12: the pairing unit's build of it
    (linear chains, BN_CYC_LIN) on the structured rows"""
    same(opctx.fq12_op_many("cyc_sqr", rows["a"]), rows["cyc_a"], "cyc_sqr")


def test_op_unit_rejects_other_values(ctx):
    from substrate_bn import BnError
    with pytest.raises(BnError):
        ctx.set_fq12_op_unit(2)


@pytest.mark.parametrize("n", [1, 33, 257])
def test_pairing_full(ctx_tp, ref, n):
    """k_pairing_full: the Miller loop's Fq12 squarings and the final exponentiation's
    products; a zero G1, a zero G2 and a z == one row in the tail"""
    p, q, want = ref["p"][:n].copy(), ref["q"][:n].copy(), ref["gt"][:n].copy()
    if n > 3:
        one = O.canon_to_mont_array([1])
        p[n - 1] = 0
        p[n - 1, 4:8] = one              # G1::zero()
        q[n - 2] = 0
        q[n - 2, 8:12] = one             # G2::zero(): y = (1, 0)
        want[n - 1] = want[n - 2] = O.canon_to_mont_array(ONE12)
        p[n - 3], q[n - 3], want[n - 3] = ref["pa"][0], ref["qa"][0], ref["gta"][0]
    same(ctx_tp.pairing_many(p, q), want, "pairing_many")


@pytest.mark.parametrize("n", [5, 64])
def test_pairing_batch(ctx, ref, n):
    """k_miller_seg's squarings: one product of n pairings"""
    p, q = ref["p"][:n], ref["q"][:n]
    assert np.array_equal(ctx.pairing_batch(p, q), O.pairing_batch(p, q, nthreads=NT))
