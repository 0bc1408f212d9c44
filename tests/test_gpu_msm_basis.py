"""One large G1 MSM over a fixed basis at the C ABI (bn_g1_basis_prepare, bn_g1_msm_basis,
bn_g1_msm_basis_dev) against the oracle, bit for bit on the 12 words of the normalized image,
and against bn_g1_msm on the same slice.  The expected value is the oracle's alone: O.g1_mul of
every term, a halving tree of O.g1_add, O.g1_normalize; a zero sum is the (0, one, 0) image."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_basis_cases as C

pytestmark = pytest.mark.gpu
NT = C.NT
R = C.R
SIZES = [0, 1, 2, 63, 64, 65, 257, 1000, 4099]
WIDTHS = [2, 5, 0]
NMAX = 4099
PATTERN = 0x5a5a


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    c = Context(0)
    c.set_msm_min(0)
    return c


@pytest.fixture(scope="module")
def pool():
    """NMAX bases and scalars and their oracle products, computed once and shared."""
    p = C.g1_points(NMAX, 7001)
    assert not np.array_equal(p[0, 8:12], O.canon_to_mont_array([1]).reshape(4))  # Jacobian, z != one
    _, k = O.random_scalars(NMAX, seed=7002, lo=0)
    prod = O.g1_mul(p, k, nthreads=NT)
    for a in (p, k, prod):
        a.setflags(write=False)
    return {"p": p, "k": k, "prod": prod}


@pytest.fixture(scope="module")
def bases(ctx, pool):
    """The pool's NMAX bases prepared once per width."""
    import substrate_bn as bn
    hs = {c: bn.G1Basis(pool["p"], window=c, ctx=ctx) for c in WIDTHS}
    yield hs
    for h in hs.values():
        h.close()


def _to_dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).reshape(-1)).to(torch.device("cuda", 0))


def _dev(ctx, handle, k):
    import torch
    dev = torch.device("cuda", 0)
    n = k.shape[0]
    K = _to_dev(k) if n else torch.zeros(4, dtype=torch.int64, device=dev)
    out = torch.full((12,), PATTERN, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g1_msm_basis_dev(handle, K.data_ptr(), n, out.data_ptr())
    ctx.dev_status()  # synchronizes the context's stream
    return out.cpu().numpy().view(np.uint64)


def _check(ctx, basis, k, want):
    k = np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)
    h = basis._handle()
    assert np.array_equal(ctx.g1_msm_basis(h, k), want), "host form"
    assert np.array_equal(_dev(ctx, h, k), want), "device form"


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, pool, bases, n, c):
    b = bases[c]
    assert len(b) == NMAX and b.count == NMAX and (b.window == c if c else 2 <= b.window <= 16)
    want = C.expect_from_products(pool["prod"][:n])
    _check(ctx, b, pool["k"][:n], want)
    assert np.array_equal(ctx.g1_msm(pool["p"][:n], pool["k"][:n]), want)  # bn_g1_msm on the same slice


@pytest.mark.parametrize("c", [11, 16])
def test_wide_windows(ctx, pool, c):
    """c = 16: 2^19 keys, mostly empty buckets, a top window of 14 bits; c = 11: of one bit."""
    import substrate_bn as bn
    n = 257
    with bn.G1Basis(pool["p"][:n], window=c, ctx=ctx) as b:
        assert b.window == c
        want = C.expect_from_products(pool["prod"][:n])
        _check(ctx, b, pool["k"][:n], want)
        assert np.array_equal(ctx.g1_msm(pool["p"][:n], pool["k"][:n]), want)
        _check(ctx, b, pool["k"][:64], C.expect_from_products(pool["prod"][:64]))


def test_run_split_with_mixed_additions(ctx, pool, bases):
    n = 1000
    want = C.expect_from_products(pool["prod"][:n])
    try:
        for cap in (4, 1):                         # 1: three fold levels
            ctx.set_msm_run_max(cap)
            for c in (5, 0):
                _check(ctx, bases[c], pool["k"][:n], want)
    finally:
        ctx.set_msm_run_max(0)
    n = 4096                                       # all scalars equal: one bucket per window holds every term
    k = np.ascontiguousarray(np.broadcast_to(pool["k"][5], (n, 4)))
    want = C.expect(pool["p"][:n], k)
    for c in WIDTHS:
        _check(ctx, bases[c], k, want)


@pytest.mark.parametrize("c", [2, 5, 11])
def test_planted_rows(ctx, pool, c):
    import substrate_bn as bn
    n = 257
    p, k = C.planted(pool["p"][:n], pool["k"][:n], c)
    want = C.expect(p, k)
    with bn.G1Basis(p, window=c, ctx=ctx) as b:
        _check(ctx, b, k, want)
        assert np.array_equal(ctx.g1_msm(p, k), want)
        try:
            ctx.set_msm_run_max(4)
            _check(ctx, b, k, want)
        finally:
            ctx.set_msm_run_max(0)


@pytest.mark.parametrize("nbases", [1, 64, 65])
def test_table_rows_at_the_edges_of_the_build_wave(ctx, pool, nbases):
    import substrate_bn as bn
    with bn.G1Basis(pool["p"][:nbases], window=5, ctx=ctx) as b:
        assert len(b) == nbases
        _check(ctx, b, pool["k"][:nbases], C.expect_from_products(pool["prod"][:nbases]))
    # prepared from device memory
    P = _to_dev(pool["p"][:nbases])
    import torch
    torch.cuda.synchronize()
    with bn.G1Basis(P.data_ptr(), window=5, ctx=ctx, count=nbases) as b:
        assert len(b) == nbases and b.window == 5
        _check(ctx, b, pool["k"][:nbases], C.expect_from_products(pool["prod"][:nbases]))


def test_python_front_end(ctx, pool, bases):
    import substrate_bn as bn
    n = 65
    got = bn.g1_msm_basis(bases[5], pool["k"][:n])
    assert isinstance(got, bn.G1) and np.array_equal(got.img, C.expect_from_products(pool["prod"][:n]))
    assert np.array_equal(bn.g1_msm_basis(bases[5], []).img, C.zero())
    ctx.g1_msm_basis_reserve(bases[5]._handle(), NMAX)
    ctx.g1_msm_basis_reserve(bases[5]._handle(), 0)


def test_lifecycle_and_refusals(ctx, pool, bases):
    from substrate_bn import BnError, Context, _native
    L, h = _native.load(), ctx.handle
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    vp = ctypes.c_void_p
    out = np.zeros(12, np.uint64)
    po, pp, pk = (vp(a.ctypes.data) for a in (out, pool["p"], pool["k"]))
    new = vp(0x1234)
    # the prepare call: refused before anything is read, *out untouched
    assert L.bn_g1_basis_prepare(h, None, 4, 5, ctypes.byref(new)) == INVALID
    assert L.bn_g1_basis_prepare(h, pp, 4, 5, None) == INVALID
    assert L.bn_g1_basis_prepare(h, pp, 0, 5, ctypes.byref(new)) == INVALID
    assert L.bn_g1_basis_prepare(h, pp, (1 << 26) + 1, 16, ctypes.byref(new)) == INVALID
    assert L.bn_g1_basis_prepare(h, pp, (2 ** 31 - 1) // 128 + 1, 2, ctypes.byref(new)) == INVALID  # nbases * W(2) over 2^31 - 1
    for c in (-1, 1, 17, 64):
        assert L.bn_g1_basis_prepare(h, pp, 4, c, ctypes.byref(new)) == INVALID
        assert L.bn_g1_basis_prepare_dev(h, pp, 4, c, ctypes.byref(new), None) == INVALID
    assert L.bn_g1_basis_prepare_dev(h, None, 4, 5, ctypes.byref(new), None) == INVALID
    assert new.value == 0x1234
    # the MSM call
    b5 = vp(bases[5]._handle())
    assert L.bn_g1_msm_basis(h, None, pk, 4, po) == INVALID
    assert L.bn_g1_msm_basis(h, b5, None, 4, po) == INVALID
    assert L.bn_g1_msm_basis(h, b5, pk, 4, None) == INVALID
    assert L.bn_g1_msm_basis(h, b5, pk, NMAX + 1, po) == INVALID
    assert L.bn_g1_msm_basis_dev(h, b5, pk, NMAX + 1, po, None) == INVALID
    assert L.bn_g1_msm_basis_dev(h, b5, None, 4, po, None) == INVALID
    assert L.bn_g1_msm_basis_dev(h, None, pk, 4, po, None) == INVALID
    assert L.bn_g1_msm_basis_reserve(h, b5, NMAX + 1) == INVALID
    assert L.bn_g1_msm_basis_reserve(h, None, 4) == INVALID
    assert L.bn_g1_basis_destroy(h, None) == INVALID
    assert not out.any()
    # a second context refuses the handle; the context that owns it goes on working
    other = Context(0)
    assert L.bn_g1_msm_basis(other.handle, b5, pk, 4, po) == INVALID
    assert L.bn_g1_basis_destroy(other.handle, b5) == INVALID
    assert L.bn_g1_msm_basis_reserve(other.handle, b5, 4) == INVALID
    other.close()
    want = C.expect_from_products(pool["prod"][:65])
    _check(ctx, bases[5], pool["k"][:65], want)
    # a destroyed handle is refused (looked up, never dereferenced)
    dead = ctx.g1_basis_prepare(pool["p"][:3], 5)
    assert ctx.g1_basis_count(dead) == 3 and ctx.g1_basis_window(dead) == 5
    ctx.g1_basis_destroy(dead)
    assert L.bn_g1_msm_basis(h, vp(dead), pk, 3, po) == INVALID
    assert L.bn_g1_basis_destroy(h, vp(dead)) == INVALID
    with pytest.raises(BnError) as e:
        ctx.g1_msm_basis_dev(dead, 0, 0, 0)
    assert e.value.code == INVALID
    # two live handles of different widths used alternately
    for _ in range(2):
        for c in (2, 0, 5):
            assert np.array_equal(ctx.g1_msm_basis(bases[c]._handle(), pool["k"][:65]), want), c
    # a multi-device context refuses; its device context works
    mctx = Context(devices=[0, 0])
    assert L.bn_g1_basis_prepare(mctx.handle, pp, 4, 5, ctypes.byref(new)) == INVALID and new.value == 0x1234
    assert L.bn_g1_msm_basis(mctx.handle, b5, pk, 4, po) == INVALID
    assert L.bn_g1_msm_basis_reserve(mctx.handle, b5, 4) == INVALID
    sub = vp(L.bn_ctx_device(mctx.handle, 0))
    made = vp()
    assert L.bn_g1_basis_prepare(sub, pp, 65, 5, ctypes.byref(made)) == 0 and made.value
    assert L.bn_g1_msm_basis(sub, made, pk, 65, po) == 0
    assert np.array_equal(out, want)
    assert L.bn_g1_basis_destroy(sub, made) == 0
    mctx.close()


def test_a_context_frees_its_live_handles(pool):
    from substrate_bn import Context
    c = Context(0)
    h = c.g1_basis_prepare(pool["p"][:65], 5)
    assert np.array_equal(c.g1_msm_basis(h, pool["k"][:65]), C.expect_from_products(pool["prod"][:65]))
    c.close()                                      # the handle is still alive


def test_sequencing_on_one_stream(ctx, pool, bases):
    """bn_g1_msm_basis_dev, bn_pairing_batch_dev, bn_g1_msm_basis_dev on one caller stream with no
    host synchronization between them, then bn_g1_msm_dev between two basis calls: the shared
    MSM workspace."""
    import torch
    n = 257
    dev = torch.device("cuda", 0)
    p, q, _, _ = O.random_pairs(3, seed=7004, nthreads=NT)
    h = bases[0]._handle()
    ctx.g1_msm_basis_reserve(h, n)
    m_alone = ctx.g1_msm_basis(h, pool["k"][:n])
    assert np.array_equal(m_alone, C.expect_from_products(pool["prod"][:n]))
    pb_alone = ctx.pairing_batch(p, q)
    assert np.array_equal(pb_alone, O.pairing_batch(p, q))
    half_alone = ctx.g1_msm(pool["p"][:100], pool["k"][:100])
    assert np.array_equal(half_alone, C.expect_from_products(pool["prod"][:100]))
    P, K, P3, Q3 = _to_dev(pool["p"][:n]), _to_dev(pool["k"][:n]), _to_dev(p), _to_dev(q)
    o = [torch.full((12,), PATTERN, dtype=torch.int64, device=dev) for _ in range(4)]
    o2 = torch.zeros(48, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ctx.g1_msm_basis_dev(h, K.data_ptr(), n, o[0].data_ptr(), s.cuda_stream)
    ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, o2.data_ptr(), None, s.cuda_stream)
    ctx.g1_msm_basis_dev(h, K.data_ptr(), n, o[1].data_ptr(), s.cuda_stream)
    ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), 100, o[2].data_ptr(), s.cuda_stream)
    ctx.g1_msm_basis_dev(bases[5]._handle(), K.data_ptr(), n, o[3].data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(dev)
    got = [t.cpu().numpy().view(np.uint64) for t in o]
    assert np.array_equal(got[0], m_alone) and np.array_equal(got[1], m_alone) and np.array_equal(got[3], m_alone)
    assert np.array_equal(o2.cpu().numpy().view(np.uint64), pb_alone)
    assert np.array_equal(got[2], half_alone)
