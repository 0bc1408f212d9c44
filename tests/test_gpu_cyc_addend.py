"""The split-layout cyclotomic square on the addend-taking column sums (tower.h
fq12_cyclotomic_sqr, fq2_split.h fq2_cyc_u / fq_dot2_add) through every kernel that
runs it -- k_fq12_vm (cyc_sqr, exp_by_neg_z), k_gt_pow and the throughput path's
k_pairing_full -- bit for bit against the oracle.  The formula is defined for any
Fq12, so the square is also run on zero, one, all coordinates p - 1 and elements
with one Fq2 coefficient zeroed.  tests/test_column_asm_addend.py checks the chain's
text instruction by instruction on the CPU.
Runs on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
NT = 16
NPAIR = 257
ONE12 = O.canon_to_mont_array([1] + [0] * 11)


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def ctx_tp():
    """Every pairing_many batch on the throughput path (k_pairing_full, the kernel
    bench.py's headline measures): the latency-path threshold is 0."""
    from substrate_bn import Context
    c = Context(0)
    c.set_fe_wide_max(0)
    return c


@pytest.fixture(scope="module")
def ref():
    """257 random pairs in Jacobian form (z != one on both sides) and the generators
    (z == one), with the oracle's Gt of each: computed once, read-only."""
    _, S = O.random_scalars(NPAIR, seed=9091, lo=1)
    p = O.g1_mul(np.tile(O.g1_one(), (NPAIR, 1)), S, NT)
    q = O.g2_mul(np.tile(O.g2_one(), (NPAIR, 1)), np.roll(S, 3, axis=0), NT)
    pa, qa = np.array(O.g1_one()).reshape(1, 12), np.array(O.g2_one()).reshape(1, 24)
    d = {"p": p, "q": q, "gt": O.pairing_many(p, q, NT), "pa": pa, "qa": qa, "gta": O.pairing_many(pa, qa)}
    for v in d.values():
        v.setflags(write=False)
    return d


def rnd_fq12(n, seed):
    g = O.SplitMix64(seed)
    return O.canon_to_mont_array([g.below(O.P) for _ in range(12 * n)]).reshape(n, 48)


@pytest.fixture(scope="module")
def rows(ref):
    """128 Fq12 rows: 0, 1, all coordinates p - 1, six random elements with Fq2
    coefficient 0..5 zeroed (either member of every pair (z0, z1), (z2, z3), (z4, z5)),
    32 pairing outputs, random fill."""
    edge = np.zeros((9, 48), np.uint64)
    edge[1] = ONE12
    edge[2] = O.canon_to_mont_array([O.P - 1] * 12)
    edge[3:9] = rnd_fq12(6, 31)
    for k in range(6):
        edge[3 + k, 8 * k:8 * k + 8] = 0
    a = np.concatenate([edge, ref["gt"][:32], rnd_fq12(128 - 9 - 32, 32)])
    assert a.shape == (128, 48)
    a.setflags(write=False)
    return a


def test_cyc_sqr_rows(ctx, rows):
    got = ctx.fq12_op_many("cyc_sqr", rows)
    want = O.unary("orc_fq12_cyclotomic_squared", rows, 48)[0]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "rows %s differ" % bad[:8]


def test_exp_by_neg_z_rows(ctx, rows):
    a = rows[:16]  # the nine edge rows and seven pairing outputs
    assert np.array_equal(ctx.fq12_op_many("exp_by_neg_z", a), O.unary("orc_fq12_exp_by_neg_z", a, 48)[0])


def test_gt_pow_rows(ctx, ref):
    """64 pairing outputs: every wave of k_gt_pow takes the cyclotomic squarings"""
    a = ref["gt"][:64]
    _, K = O.random_scalars(64, seed=9093, lo=0)
    assert np.array_equal(ctx.gt_pow_many(a, K), O.gt_pow(a, K))


@pytest.mark.parametrize("n", [1, 31, 33, 255, 257])
def test_pairing_full_ragged(ctx_tp, ref, n):
    """k_pairing_full at sizes that leave waves (32 pairs) and blocks (256 pairs)
    ragged; Jacobian inputs with a zero G1, a zero G2 and a z == one row in the tail"""
    p, q, want = ref["p"][:n].copy(), ref["q"][:n].copy(), ref["gt"][:n].copy()
    if n > 3:
        one = O.canon_to_mont_array([1])
        p[n - 1] = 0
        p[n - 1, 4:8] = one              # G1::zero()
        q[n - 2] = 0
        q[n - 2, 8:12] = one             # G2::zero(): y = (1, 0)
        want[n - 1] = want[n - 2] = ONE12
        p[n - 3], q[n - 3], want[n - 3] = ref["pa"][0], ref["qa"][0], ref["gta"][0]
    got = ctx_tp.pairing_many(p, q)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "rows %s of %d differ" % (bad[:8], n)
