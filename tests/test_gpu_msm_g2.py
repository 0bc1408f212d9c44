"""G2 multi-scalar multiplication at the C ABI (bn_g2_msm, bn_g2_msm_dev) against the
oracle, bit for bit on the 24 words of the normalized image.  The expected value is
the oracle's alone (tests/msm_g2_cases.py): O.g2_mul of every term, a halving tree of
O.g2_add, O.g2_normalize; a zero sum is the (0, one, 0) image.  Every case runs the
bucket path at window widths 2, 5 and automatic (bn_set_msm_min(0), so it runs at any
n), the small path, and the device-pointer form; all must give the same 192 bytes."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_g2_cases as C

pytestmark = pytest.mark.gpu
NT = C.NT
R = C.R
SIZES = [0, 1, 2, 3, 63, 64, 65, 257, 1000, 1031]
NMAX = 1031
CAP = 1 << 26  # bn_g2_msm's documented cap on n


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def pool():
    """NMAX points and scalars and their oracle products, computed once and shared."""
    _, small, _, _ = O.random_pairs(8, seed=7001, nthreads=NT)
    p = C.g2_points(NMAX, 7001)
    assert np.array_equal(C.g2_points(8, 7001), small)  # the helper is random_pairs' G2 half
    one = np.zeros(8, np.uint64)
    one[:4] = O.canon_to_mont_array([1]).reshape(4)
    assert not np.array_equal(p[0, 16:24], one)  # Jacobian, z != one
    _, k = O.random_scalars(NMAX, seed=7002, lo=0)
    p.setflags(write=False)
    k.setflags(write=False)
    prod = O.g2_mul(p, k, nthreads=NT)
    prod.setflags(write=False)
    return {"p": p, "k": k, "prod": prod}


def _dev(ctx, p, k):
    import torch
    dev = torch.device("cuda", 0)
    n = p.shape[0]
    # copies: the shared pool is read-only; with no terms the pointers are still valid ones
    P = torch.from_numpy(np.array(p, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev) if n else torch.zeros(24, dtype=torch.int64, device=dev)
    K = torch.from_numpy(np.array(k, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev) if n else torch.zeros(4, dtype=torch.int64, device=dev)
    out = torch.full((24,), 0x5a5a, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g2_msm_dev(P.data_ptr(), K.data_ptr(), n, out.data_ptr())
    ctx.dev_status()  # synchronizes the context's stream
    return out.cpu().numpy().view(np.uint64)


def _all_ways(ctx, p, k):
    """{name: 24 words} of the same MSM by the bucket path at windows 2, 5 and automatic,
    the small path and the device-pointer form."""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 24)
    k = np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)
    got = {}
    try:
        ctx.set_msm_min(0)
        for c in (2, 5, 0):
            ctx.set_msm_window(c)
            got["bucket c=%d" % c] = ctx.g2_msm(p, k)
        got["dev"] = _dev(ctx, p, k)
        ctx.set_msm_min(p.shape[0] + 1)
        got["small"] = ctx.g2_msm(p, k)
    finally:
        ctx.set_msm_window(0)
        ctx.set_msm_min(0)
    return got


def _check(ctx, p, k, want):
    for name, out in _all_ways(ctx, p, k).items():
        assert np.array_equal(out, want), name


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, pool, n):
    _check(ctx, pool["p"][:n], pool["k"][:n], C.expect_from_products(pool["prod"][:n]))


def test_planted_cases(ctx, pool):
    n = 257
    p, k = C.plant(pool["p"][:n], pool["k"][:n], lambda nw: (1, 3, nw // 2, nw - 1))
    _check(ctx, p, k, C.expect(p, k))


def test_all_scalars_equal(ctx, pool):
    n = 1024                                   # one bucket per window holds every term
    p = pool["p"][:n]
    k = np.ascontiguousarray(np.broadcast_to(pool["k"][5], (n, 4)))
    _check(ctx, p, k, C.expect(p, k))


def test_small_scalars(ctx, pool):
    n = 1000                                   # most windows empty
    rng = np.random.default_rng(5)
    k = C.fr([int(v) for v in rng.integers(0, 1 << 16, n)])
    _check(ctx, pool["p"][:n], k, C.expect(pool["p"][:n], k))


def test_all_scalars_zero(ctx, pool):
    n = 300
    _check(ctx, pool["p"][:n], np.zeros((n, 4), np.uint64), C.zero())


def test_pair_that_cancels(ctx, pool):
    kv = 0x1f2e3d4c5b6a79880123456789abcdef
    p = np.stack([pool["p"][17], pool["p"][17]])
    k = C.fr([kv, R - kv])
    assert np.array_equal(C.expect(p, k), C.zero())
    _check(ctx, p, k, C.zero())


def test_one_term_at_the_last_index(ctx, pool):
    n = 1000
    k = np.zeros((n, 4), np.uint64)
    k[n - 1] = pool["k"][n - 1]
    want = O.g2_normalize(pool["prod"][n - 1:n])[0]
    assert np.array_equal(want, C.expect(pool["p"][:n], k))
    _check(ctx, pool["p"][:n], k, want)


def test_normalized_inputs(ctx, pool):
    n = 65
    p = O.g2_normalize(pool["p"][:n])         # z == one
    assert np.array_equal(p[:, 16:24], np.broadcast_to(C.zero()[8:16], (n, 8)))
    want = C.expect(p, pool["k"][:n])
    assert np.array_equal(want, C.expect_from_products(pool["prod"][:n]))  # the same point, so the same image
    _check(ctx, p, pool["k"][:n], want)


def test_permutation_and_linearity(ctx, pool):
    n = 1000
    p, k = pool["p"][:n], pool["k"][:n]
    ctx.set_msm_min(0)
    base = ctx.g2_msm(p, k)
    perm = np.random.default_rng(11).permutation(n)
    assert np.array_equal(ctx.g2_msm(p[perm], k[perm]), base)
    kv, k2 = O.random_scalars(n, seed=7003, lo=0)
    kc = O.mont_array_to_canon(k.reshape(-1), O.FR)
    ksum = C.fr([int(a) + int(b) for a, b in zip(kc, kv)])
    lhs = ctx.group_op_many("g2", "add", base, ctx.g2_msm(p, k2))
    rhs = ctx.g2_msm(p, ksum)
    assert ctx.group_op_many("g2", "eq", lhs, rhs)[0] == 1
    assert ctx.group_op_many("g2", "eq", lhs, base)[0] == 0  # the comparison can fail


def test_multi_device(ctx, pool):
    from substrate_bn import BnError, Context
    mctx = Context(devices=[0, 0])
    ctx.set_msm_min(0)
    mctx.set_msm_min(0)
    for n in (1, 5, 1031):
        p, k = pool["p"][:n], pool["k"][:n]
        want = C.expect_from_products(pool["prod"][:n])
        assert np.array_equal(ctx.g2_msm(p, k), want), n
        assert np.array_equal(mctx.g2_msm(p, k), want), n
    mctx.set_msm_min(1 << 20)                 # the shards on the small path
    for n in (1, 5, 1031):
        assert np.array_equal(mctx.g2_msm(pool["p"][:n], pool["k"][:n]), C.expect_from_products(pool["prod"][:n])), n
    assert np.array_equal(mctx.g2_msm(pool["p"][:0], pool["k"][:0]), C.zero())
    with pytest.raises(BnError) as e:
        mctx.g2_msm_dev(0, 0, 0, 0)
    assert e.value.code == 1
    # the cap on n holds for the whole sum, before any shard reads a buffer
    import ctypes
    from substrate_bn import _native
    out = np.zeros(24, np.uint64)
    po, pp, pk = (ctypes.c_void_p(a.ctypes.data) for a in (out, pool["p"], pool["k"]))
    assert _native.load().bn_g2_msm(mctx.handle, pp, pk, CAP + 1, po) == _native.BN_ERR_INVALID_ARGUMENT
    assert np.array_equal(mctx.g2_msm(pool["p"][:5], pool["k"][:5]), C.expect_from_products(pool["prod"][:5]))
    mctx.close()


def test_argument_checks(ctx, pool):
    import ctypes
    from substrate_bn import BnError, _native
    L, h = _native.load(), ctx.handle
    out = np.zeros(24, np.uint64)
    po, pp, pk = (ctypes.c_void_p(a.ctypes.data) for a in (out, pool["p"], pool["k"]))
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    assert L.bn_g2_msm(h, None, pk, 4, po) == INVALID
    assert L.bn_g2_msm(h, pp, None, 4, po) == INVALID
    assert L.bn_g2_msm(h, pp, pk, 4, None) == INVALID
    assert L.bn_g2_msm_dev(h, None, None, 4, None, None) == INVALID
    assert L.bn_g2_msm(h, pp, pk, CAP + 1, po) == INVALID        # refused before any buffer is read
    assert L.bn_g2_msm_dev(h, pp, pk, CAP + 1, po, None) == INVALID
    assert L.bn_g2_msm_reserve(h, CAP + 1) == INVALID
    ctx.set_msm_window(2)                      # n * W(2) = 2^24 * 128 > 2^31 - 1
    try:
        assert L.bn_g2_msm_reserve(h, 1 << 24) == INVALID
    finally:
        ctx.set_msm_window(0)
    for c in (-1, 1, 17, 64):
        with pytest.raises(BnError) as e:
            ctx.set_msm_window(c)
        assert e.value.code == INVALID
    # the context stays usable, at its previous settings
    ctx.set_msm_min(0)
    assert np.array_equal(ctx.g2_msm(pool["p"][:65], pool["k"][:65]), C.expect_from_products(pool["prod"][:65]))


def test_shared_workspace_with_g1_and_pairing_batch(ctx, pool):
    """The uint32 buffers are shared with bn_g1_msm: interleaved calls, and a caller
    stream of _dev calls with no host sync in between, return what each returns alone."""
    n = 257
    p, q, _, _ = O.random_pairs(3, seed=7004, nthreads=NT)
    _, s1 = O.random_scalars(n, 7005)
    p1 = O.g1_mul(O.g1_one(), s1, NT)
    k1 = pool["k"][:n]
    ctx.set_msm_min(0)
    ctx.msm_reserve(n)
    ctx.g2_msm_reserve(n)
    g2_alone = ctx.g2_msm(pool["p"][:n], k1)
    g1_alone = ctx.g1_msm(p1, k1)
    pb_alone = ctx.pairing_batch(p, q)
    assert np.array_equal(g2_alone, C.expect_from_products(pool["prod"][:n]))
    assert np.array_equal(pb_alone, O.pairing_batch(p, q))
    g1_want = O.g1_mul(p1, k1, nthreads=NT)
    while g1_want.shape[0] > 1:
        h = (g1_want.shape[0] + 1) // 2
        m = g1_want.shape[0] - h
        g1_want = np.concatenate([O.g1_add(g1_want[:m], g1_want[h:]), g1_want[m:h]])
    assert np.array_equal(g1_alone, O.g1_normalize(g1_want)[0])
    a = ctx.g1_msm(p1, k1)
    b = ctx.g2_msm(pool["p"][:n], k1)
    c = ctx.g1_msm(p1, k1)
    assert np.array_equal(a, g1_alone) and np.array_equal(b, g2_alone) and np.array_equal(c, g1_alone)
    import torch
    dev = torch.device("cuda", 0)

    def up(a):
        return torch.from_numpy(np.array(a).view(np.int64)).to(dev)

    P2, P1, K, P3, Q3 = up(pool["p"][:n]), up(p1), up(k1), up(p), up(q)
    o1 = torch.zeros(24, dtype=torch.int64, device=dev)
    o2 = torch.zeros(48, dtype=torch.int64, device=dev)
    o3 = torch.zeros(12, dtype=torch.int64, device=dev)
    o4 = torch.zeros(24, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ctx.g2_msm_dev(P2.data_ptr(), K.data_ptr(), n, o1.data_ptr(), s.cuda_stream)
    ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, o2.data_ptr(), None, s.cuda_stream)
    ctx.g1_msm_dev(P1.data_ptr(), K.data_ptr(), n, o3.data_ptr(), s.cuda_stream)
    ctx.g2_msm_dev(P2.data_ptr(), K.data_ptr(), n, o4.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(o1.cpu().numpy().view(np.uint64), g2_alone)
    assert np.array_equal(o2.cpu().numpy().view(np.uint64), pb_alone)
    assert np.array_equal(o3.cpu().numpy().view(np.uint64), g1_alone)
    assert np.array_equal(o4.cpu().numpy().view(np.uint64), g2_alone)
