"""G2 multi-scalar multiplication over skewed scalars at the C ABI (bn_g2_msm,
bn_g2_msm_dev) with the run cap forced (bn_set_msm_run_max), so that small batches reach
the two-lane chunk and fold kernels: L = 1 at n = 33 / 1025 gives two / three ragged fold
levels at fan-in 32.  The expected value is the oracle's alone (tests/msm_skew_cases.py),
bit for bit on the 24 words of the normalized image, the same at every cap and window
width."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_skew_cases as C

pytestmark = pytest.mark.gpu
GROUP = "g2"
SIZES = [1, 2, 3, 33, 65, 1025]
NMAX = 1025


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def pool():
    """NMAX points, uniform scalars and their oracle products, computed once and shared."""
    g = C.Group(GROUP)
    pts = g.points(NMAX, 7501)
    _, k = O.random_scalars(NMAX, seed=7502, lo=0)
    prod = g.mul(pts, k, C.NT)
    for a in (pts, k, prod):
        a.setflags(write=False)
    return g, pts, k, prod


def _case(pool, pattern, n):
    g, pts, k, prod = pool
    return C.case(g, pattern, pts[:n], k[:n], prod[:n])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", C.PATTERNS)
def test_patterns_at_every_cap_and_window(ctx, pool, pattern, n):
    p, k, want = _case(pool, pattern, n)
    for key, out in C.all_settings(ctx, GROUP, p, k).items():
        assert np.array_equal(out, want), key


@pytest.mark.parametrize("n", [33, 1025])
@pytest.mark.parametrize("pattern", ["a_equal", "b_minus_ones", "d_cancelling", "f_two_hot"])
def test_dev_form(ctx, pool, pattern, n):
    p, k, want = _case(pool, pattern, n)
    try:
        ctx.set_msm_min(0)
        for c, cap in ((5, 1), (0, 3), (2, 0)):
            ctx.set_msm_window(c)
            C.set_cap(ctx, cap)
            assert np.array_equal(C.dev_form(ctx, GROUP, p, k), want), (c, cap)
    finally:
        ctx.set_msm_window(0)
        ctx.set_msm_run_max(0)


def test_uniform_scalars_at_forced_caps(ctx, pool):
    g, pts, k, prod = pool
    for n in (65, 1025):
        want = g.image(g.tree(prod[:n]))
        for key, out in C.all_settings(ctx, GROUP, pts[:n], k[:n], windows=[2, 5, 0]).items():
            assert np.array_equal(out, want), (n, key)


def test_reserve_after_the_setter(pool):
    """bn_g2_msm_reserve sizes the partial sums for the cap in force; the calls behind it,
    and calls at other settings that grow them on first use, return the same bytes."""
    from substrate_bn import Context
    c2 = Context(0)
    n = 1025
    p, k, want = _case(pool, "f_two_hot", n)
    try:
        c2.set_msm_min(0)
        c2.set_msm_run_max(1)
        c2.g2_msm_reserve(n)
        assert np.array_equal(c2.g2_msm(p, k), want)
        c2.set_msm_window(2)                   # more entries than reserved: grown on first use
        assert np.array_equal(c2.g2_msm(p, k), want)
    finally:
        c2.close()


def test_multi_device(pool):
    """The setter reaches every device; the shards' partial sums go through the split."""
    from substrate_bn import Context
    mctx = Context(devices=[0, 0])
    n = 1025
    try:
        mctx.set_msm_min(0)
        p, k, want = _case(pool, "a_equal", n)
        for cap in (1, 64, 0):
            mctx.set_msm_run_max(cap)
            assert np.array_equal(mctx.g2_msm(p, k), want), cap
    finally:
        mctx.close()
