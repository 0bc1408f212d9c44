"""G1 multi-scalar multiplication over skewed scalars at the C ABI (bn_g1_msm,
bn_g1_msm_dev) with the run cap forced (bn_set_msm_run_max), so that small batches reach
the chunk and fold kernels: L = 1 at n = 33 / 1025 / 4099 gives two / three / three ragged
fold levels at fan-in 32.  The expected value is the oracle's alone
(tests/msm_skew_cases.py), bit for bit on the 12 words of the normalized image, the same at
every cap and window width."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_skew_cases as C

pytestmark = pytest.mark.gpu
GROUP = "g1"
SIZES = [1, 2, 3, 33, 65, 1025, 4099]
NMAX = 4099


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def pool():
    """NMAX points, uniform scalars and their oracle products, computed once and shared."""
    g = C.Group(GROUP)
    pts = g.points(NMAX, 7401)
    _, k = O.random_scalars(NMAX, seed=7402, lo=0)
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
    for n in (65, 4099):
        want = g.image(g.tree(prod[:n]))
        for key, out in C.all_settings(ctx, GROUP, pts[:n], k[:n], windows=[2, 5, 0]).items():
            assert np.array_equal(out, want), (n, key)


def test_setter_refusals(ctx, pool):
    from substrate_bn import BnError, _native
    for bad in ((1 << 16) + 1, 1 << 20, _native.MSM_RUN_UNSPLIT - 1):
        with pytest.raises(BnError) as e:
            ctx.set_msm_run_max(bad)
        assert e.value.code == _native.BN_ERR_INVALID_ARGUMENT
    assert _native.load().bn_set_msm_run_max(None, 1) != 0      # no context
    for ok in (1, 1 << 16, _native.MSM_RUN_UNSPLIT, 0):
        ctx.set_msm_run_max(ok)
    # the context stays usable, at the default
    p, k, want = _case(pool, "a_equal", 65)
    ctx.set_msm_min(0)
    assert np.array_equal(ctx.g1_msm(p, k), want)


def test_setting_survives_the_many_msm_long_segment_route(ctx, pool):
    """A segment above bn_g1_msm_many's packed limit runs on bn_g1_msm's path: at the cap in
    force, leaving it in force."""
    n = 1025
    p, k, want = _case(pool, "a_equal", n)
    try:
        ctx.set_msm_min(0)
        ctx.set_msm_run_max(1)
        a = ctx.g1_msm(p, k)
        many = ctx.g1_msm_many(p, k, [0, n])
        b = ctx.g1_msm(p, k)
        ctx.set_msm_run_max(3)
        many3 = ctx.g1_msm_many(np.concatenate([p, p[:7]]), np.concatenate([k, k[:7]]), [0, n, n + 7])
    finally:
        ctx.set_msm_run_max(0)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    assert np.array_equal(many.reshape(-1, 12)[0], want)
    assert np.array_equal(many3.reshape(-1, 12)[0], want)
    g = pool[0]
    assert np.array_equal(many3.reshape(-1, 12)[1], g.image(g.times(p[:7], C.K_EQUAL)))


def test_reserve_after_the_setter(pool):
    """bn_msm_reserve sizes the partial sums for the cap in force; the calls behind it, and
    calls at other caps that grow them on first use, return the same bytes."""
    from substrate_bn import Context
    c2 = Context(0)
    n = 1025
    p, k, want = _case(pool, "f_two_hot", n)
    try:
        c2.set_msm_min(0)
        c2.set_msm_run_max(1)
        c2.msm_reserve(n)
        assert np.array_equal(c2.g1_msm(p, k), want)
        c2.set_msm_window(2)                   # more entries than reserved: grown on first use
        assert np.array_equal(c2.g1_msm(p, k), want)
        c2.set_msm_run_max(3)
        c2.msm_reserve(n)
        assert np.array_equal(c2.g1_msm(p, k), want)
    finally:
        c2.close()


def test_multi_device(pool):
    """The setter reaches every device; the shards' partial sums go through the split."""
    from substrate_bn import Context
    mctx = Context(devices=[0, 0])
    n = 1025
    try:
        mctx.set_msm_min(0)
        for pattern in ("a_equal", "f_two_hot"):
            p, k, want = _case(pool, pattern, n)
            for cap in (1, 64, 0):
                mctx.set_msm_run_max(cap)
                assert np.array_equal(mctx.g1_msm(p, k), want), (pattern, cap)
    finally:
        mctx.close()
