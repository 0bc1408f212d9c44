"""G1 multi-scalar multiplication at the C ABI (bn_g1_msm, bn_g1_msm_dev) against the
oracle, bit for bit on the 12 words of the normalized image.  The expected value is
the oracle's alone: O.g1_mul of every term, a halving tree of O.g1_add, O.g1_normalize;
a zero sum is the (0, one, 0) image.  Every case runs the bucket path at window
widths 2, 5 and automatic (bn_set_msm_min(0), so it runs at any n), the small path,
and the device-pointer form; all must give the same 96 bytes."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
NT = 16
R = O.R
SIZES = [0, 1, 2, 3, 63, 64, 65, 257, 1000, 4099]
NMAX = 4099
CAP = 1 << 26  # bn_g1_msm's documented cap on n


def _zero():
    z = np.zeros(12, np.uint64)
    z[4:8] = O.canon_to_mont_array([1]).reshape(4)  # (0, one, 0)
    return z


def _fr(vals):
    return O.canon_to_mont_array([v % R for v in vals], O.FR).reshape(len(vals), 4)


def _g1_points(n, seed):
    """The G1 half of O.random_pairs(n, seed) -- the same scalars times G1::one(), the
    same Jacobian images (z != one) -- without computing its G2 half."""
    _, s = O.random_scalars(n, seed)
    return O.g1_mul(O.g1_one(), s, NT)


def _tree(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 12).copy()
    while a.shape[0] > 1:
        h = (a.shape[0] + 1) // 2
        m = a.shape[0] - h
        a[:m] = O.g1_add(a[:m], a[h:])
        a = a[:h]
    return a


def _expect_from_products(prod):
    if prod.shape[0] == 0:
        return _zero()
    r = O.g1_normalize(_tree(prod))[0]
    return _zero() if not r[8:12].any() else r


def _expect(p, k):
    p, k = p.reshape(-1, 12), k.reshape(-1, 4)
    return _expect_from_products(O.g1_mul(p, k, nthreads=NT) if p.shape[0] else p)


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def pool():
    """NMAX points and scalars and their oracle products, computed once and shared."""
    small, _, _, _ = O.random_pairs(8, seed=7001, nthreads=NT)
    p = _g1_points(NMAX, 7001)
    assert np.array_equal(_g1_points(8, 7001), small)  # the helper is random_pairs' G1 half
    assert not np.array_equal(p[0, 8:12], O.canon_to_mont_array([1]).reshape(4))  # Jacobian, z != one
    _, k = O.random_scalars(NMAX, seed=7002, lo=0)
    p.setflags(write=False)
    k.setflags(write=False)
    prod = O.g1_mul(p, k, nthreads=NT)
    prod.setflags(write=False)
    return {"p": p, "k": k, "prod": prod}


def _dev(ctx, p, k):
    import torch
    dev = torch.device("cuda", 0)
    n = p.shape[0]
    # copies: the shared pool is read-only; with no terms the pointers are still valid ones
    P = torch.from_numpy(np.array(p, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev) if n else torch.zeros(12, dtype=torch.int64, device=dev)
    K = torch.from_numpy(np.array(k, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev) if n else torch.zeros(4, dtype=torch.int64, device=dev)
    out = torch.full((12,), 0x5a5a, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), n, out.data_ptr())
    ctx.dev_status()  # synchronizes the context's stream
    return out.cpu().numpy().view(np.uint64)


def _all_ways(ctx, p, k):
    """{name: 12 words} of the same MSM by the bucket path at windows 2, 5 and automatic,
    the small path and the device-pointer form."""
    p = np.ascontiguousarray(p, dtype=np.uint64).reshape(-1, 12)
    k = np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)
    got = {}
    try:
        ctx.set_msm_min(0)
        for c in (2, 5, 0):
            ctx.set_msm_window(c)
            got["bucket c=%d" % c] = ctx.g1_msm(p, k)
        got["dev"] = _dev(ctx, p, k)
        ctx.set_msm_min(p.shape[0] + 1)
        got["small"] = ctx.g1_msm(p, k)
    finally:
        ctx.set_msm_window(0)
        ctx.set_msm_min(0)
    return got


def _check(ctx, p, k, want):
    for name, out in _all_ways(ctx, p, k).items():
        assert np.array_equal(out, want), name


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, pool, n):
    _check(ctx, pool["p"][:n], pool["k"][:n], _expect_from_products(pool["prod"][:n]))


def test_planted_cases(ctx, pool):
    n = 257
    p, k = pool["p"][:n].copy(), pool["k"][:n].copy()
    vals = [None] * n
    z = _zero()
    p[0] = z                                   # a zero point with a nonzero scalar
    z2 = p[1].copy()
    z2[8:12] = 0                               # a zero point whose x, y are not zero's
    p[1] = z2
    vals[2] = 0                                # a nonzero point with scalar 0
    p[4], vals[3], vals[4] = p[3], 0x1234567, 0x1234567            # P twice, same scalar: doubling in a bucket
    p[6], vals[5], vals[6] = O.g1_normalize(p[5:6])[0], 99991, 99991   # P in two Jacobian scalings
    p[8], vals[7], vals[8] = O.g1_neg(p[7:8])[0], 31337, 31337      # P and -P: a bucket that cancels
    p[10] = O.g1_normalize(O.g1_neg(p[9:10]))[0]                    # -P in another scaling
    vals[9] = vals[10] = (1 << 200) + 12345
    edge = [1, R - 1, 1 << 253, R - 2, 2]
    for c in (2, 5, 10, 13, 16):               # 2^(c*w) and 2^(c*w) - 1: the digit boundaries (10: automatic at n = 257)
        nw = 254 // c + 1
        for w in (1, 3, nw // 2, nw - 1):
            if c * w < 254:
                edge += [1 << (c * w), (1 << (c * w)) - 1, (1 << (c * w - 1)), (1 << (c * w - 1)) + 1]
    assert 11 + len(edge) <= n
    for j, v in enumerate(edge):
        vals[11 + j] = v
    idx = [j for j, v in enumerate(vals) if v is not None]
    k[idx] = _fr([vals[j] for j in idx])
    _check(ctx, p, k, _expect(p, k))


def test_all_scalars_equal(ctx, pool):
    n = 4096                                   # one bucket per window holds every term
    p = pool["p"][:n]
    k = np.ascontiguousarray(np.broadcast_to(pool["k"][5], (n, 4)))
    _check(ctx, p, k, _expect(p, k))


def test_small_scalars(ctx, pool):
    n = 1000                                   # most windows empty
    rng = np.random.default_rng(5)
    k = _fr([int(v) for v in rng.integers(0, 1 << 16, n)])
    _check(ctx, pool["p"][:n], k, _expect(pool["p"][:n], k))


def test_all_scalars_zero(ctx, pool):
    n = 300
    _check(ctx, pool["p"][:n], np.zeros((n, 4), np.uint64), _zero())


def test_pair_that_cancels(ctx, pool):
    kv = 0x1f2e3d4c5b6a79880123456789abcdef
    p = np.stack([pool["p"][17], pool["p"][17]])
    k = _fr([kv, R - kv])
    assert np.array_equal(_expect(p, k), _zero())
    _check(ctx, p, k, _zero())


def test_one_term_at_the_last_index(ctx, pool):
    n = 1000
    k = np.zeros((n, 4), np.uint64)
    k[n - 1] = pool["k"][n - 1]
    want = O.g1_normalize(pool["prod"][n - 1:n])[0]
    assert np.array_equal(want, _expect(pool["p"][:n], k))
    _check(ctx, pool["p"][:n], k, want)


def test_normalized_inputs(ctx, pool):
    n = 65
    p = O.g1_normalize(pool["p"][:n])         # z == one
    assert np.array_equal(p[:, 8:12], np.broadcast_to(O.canon_to_mont_array([1]).reshape(4), (n, 4)))
    want = _expect(p, pool["k"][:n])
    assert np.array_equal(want, _expect_from_products(pool["prod"][:n]))  # the same point, so the same image
    _check(ctx, p, pool["k"][:n], want)


def test_permutation_and_linearity(ctx, pool):
    n = 1000
    p, k = pool["p"][:n], pool["k"][:n]
    ctx.set_msm_min(0)
    base = ctx.g1_msm(p, k)
    perm = np.random.default_rng(11).permutation(n)
    assert np.array_equal(ctx.g1_msm(p[perm], k[perm]), base)
    kv, k2 = O.random_scalars(n, seed=7003, lo=0)
    kc = O.mont_array_to_canon(k.reshape(-1), O.FR)
    ksum = _fr([int(a) + int(b) for a, b in zip(kc, kv)])
    lhs = ctx.group_op_many("g1", "add", base, ctx.g1_msm(p, k2))
    rhs = ctx.g1_msm(p, ksum)
    assert ctx.group_op_many("g1", "eq", lhs, rhs)[0] == 1
    assert ctx.group_op_many("g1", "eq", lhs, base)[0] == 0  # the comparison can fail


def test_multi_device(ctx, pool):
    from substrate_bn import BnError, Context
    mctx = Context(devices=[0, 0])
    ctx.set_msm_min(0)
    mctx.set_msm_min(0)
    for n in (1, 5, 4099):
        p, k = pool["p"][:n], pool["k"][:n]
        want = _expect_from_products(pool["prod"][:n])
        assert np.array_equal(ctx.g1_msm(p, k), want), n
        assert np.array_equal(mctx.g1_msm(p, k), want), n
    mctx.set_msm_min(1 << 20)                 # the shards on the small path
    assert np.array_equal(mctx.g1_msm(pool["p"][:5], pool["k"][:5]), _expect_from_products(pool["prod"][:5]))
    assert np.array_equal(mctx.g1_msm(pool["p"][:0], pool["k"][:0]), _zero())
    with pytest.raises(BnError) as e:
        mctx.g1_msm_dev(0, 0, 0, 0)
    assert e.value.code == 1
    mctx.close()


def test_argument_checks(ctx, pool):
    import ctypes
    from substrate_bn import BnError, _native
    L, h = _native.load(), ctx.handle
    out = np.zeros(12, np.uint64)
    po, pp, pk = (ctypes.c_void_p(a.ctypes.data) for a in (out, pool["p"], pool["k"]))
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    assert L.bn_g1_msm(h, None, pk, 4, po) == INVALID
    assert L.bn_g1_msm(h, pp, None, 4, po) == INVALID
    assert L.bn_g1_msm(h, pp, pk, 4, None) == INVALID
    assert L.bn_g1_msm_dev(h, None, None, 4, None, None) == INVALID
    assert L.bn_g1_msm(h, pp, pk, CAP + 1, po) == INVALID        # refused before any buffer is read
    assert L.bn_g1_msm_dev(h, pp, pk, CAP + 1, po, None) == INVALID
    assert L.bn_msm_reserve(h, CAP + 1) == INVALID
    for c in (-1, 1, 17, 64):
        with pytest.raises(BnError) as e:
            ctx.set_msm_window(c)
        assert e.value.code == INVALID
    # the context stays usable, at its previous settings
    ctx.set_msm_min(0)
    assert np.array_equal(ctx.g1_msm(pool["p"][:65], pool["k"][:65]), _expect_from_products(pool["prod"][:65]))


def test_sequencing_with_pairing_batch(ctx, pool):
    n = 257
    p, q, _, _ = O.random_pairs(3, seed=7004, nthreads=NT)
    ctx.set_msm_min(0)
    ctx.msm_reserve(n)
    m_alone = ctx.g1_msm(pool["p"][:n], pool["k"][:n])
    pb_alone = ctx.pairing_batch(p, q)
    a = ctx.g1_msm(pool["p"][:n], pool["k"][:n])
    b = ctx.pairing_batch(p, q)
    c = ctx.g1_msm(pool["p"][:n], pool["k"][:n])
    assert np.array_equal(a, m_alone) and np.array_equal(c, m_alone) and np.array_equal(b, pb_alone)
    assert np.array_equal(m_alone, _expect_from_products(pool["prod"][:n]))
    assert np.array_equal(pb_alone, O.pairing_batch(p, q))
    # the same on one caller stream with device pointers: MSM, pairing_batch, MSM, no host sync between
    import torch
    dev = torch.device("cuda", 0)
    P = torch.from_numpy(np.array(pool["p"][:n]).view(np.int64)).to(dev)
    K = torch.from_numpy(np.array(pool["k"][:n]).view(np.int64)).to(dev)
    P3 = torch.from_numpy(p.view(np.int64)).to(dev)
    Q3 = torch.from_numpy(q.view(np.int64)).to(dev)
    o1 = torch.zeros(12, dtype=torch.int64, device=dev)
    o2 = torch.zeros(48, dtype=torch.int64, device=dev)
    o3 = torch.zeros(12, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), n, o1.data_ptr(), s.cuda_stream)
    ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, o2.data_ptr(), None, s.cuda_stream)
    ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), n, o3.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(o1.cpu().numpy().view(np.uint64), m_alone)
    assert np.array_equal(o2.cpu().numpy().view(np.uint64), pb_alone)
    assert np.array_equal(o3.cpu().numpy().view(np.uint64), m_alone)
