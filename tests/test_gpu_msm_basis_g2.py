"""One large G2 MSM over a fixed basis at the C ABI (bn_g2_basis_prepare, bn_g2_msm_basis,
bn_g2_msm_basis_dev) against the oracle, bit for bit on the 24 words of the normalized image,
and against bn_g2_msm on the same slice.  The expected value is the oracle's alone
(tests/msm_g2_cases.py: O.g2_mul of every term, a halving tree of O.g2_add, O.g2_normalize; a
zero sum is the (0, one, 0) image).  Row 23 of the pool is an on-curve point outside the
order-r subgroup."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_basis_g2_cases as C

pytestmark = pytest.mark.gpu
NT = C.NT
R = C.R
SIZES = [0, 1, 2, 3, 63, 64, 65, 257, 1000, 1031]
WIDTHS = [2, 5, 0]
NMAX = 1031
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
    p = C.g2_points(NMAX, 7101)
    assert not np.array_equal(p[0, 16:20], O.canon_to_mont_array([1]).reshape(4))  # Jacobian, z != one
    p[C.OFF_AT] = C.off_subgroup_point()
    _, k = O.random_scalars(NMAX, seed=7102, lo=0)
    prod = O.g2_mul(p, k, nthreads=NT)
    for a in (p, k, prod):
        a.setflags(write=False)
    return {"p": p, "k": k, "prod": prod}


@pytest.fixture(scope="module")
def bases(ctx, pool):
    """The pool's NMAX bases prepared once per width."""
    import substrate_bn as bn
    hs = {c: bn.G2Basis(pool["p"], window=c, ctx=ctx) for c in WIDTHS}
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
    out = torch.full((24,), PATTERN, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g2_msm_basis_dev(handle, K.data_ptr(), n, out.data_ptr())
    ctx.dev_status()  # synchronizes the context's stream
    return out.cpu().numpy().view(np.uint64)


def _check(ctx, basis, k, want):
    k = np.ascontiguousarray(k, dtype=np.uint64).reshape(-1, 4)
    h = basis._handle()
    assert np.array_equal(ctx.g2_msm_basis(h, k), want), "host form"
    assert np.array_equal(_dev(ctx, h, k), want), "device form"


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, pool, bases, n, c):
    b = bases[c]
    assert len(b) == NMAX and b.count == NMAX and (b.window == c if c else 2 <= b.window <= 16)
    want = C.expect_from_products(pool["prod"][:n])
    _check(ctx, b, pool["k"][:n], want)
    assert np.array_equal(ctx.g2_msm(pool["p"][:n], pool["k"][:n]), want)  # bn_g2_msm on the same slice


@pytest.mark.parametrize("c", [11, 16])
def test_wide_windows(ctx, pool, c):
    """c = 16: 2^19 keys, mostly empty buckets, a top window of 14 bits; c = 11: of one bit."""
    import substrate_bn as bn
    n = 257
    with bn.G2Basis(pool["p"][:n], window=c, ctx=ctx) as b:
        assert b.window == c
        want = C.expect_from_products(pool["prod"][:n])
        _check(ctx, b, pool["k"][:n], want)
        assert np.array_equal(ctx.g2_msm(pool["p"][:n], pool["k"][:n]), want)
        _check(ctx, b, pool["k"][:64], C.expect_from_products(pool["prod"][:64]))


def test_run_split_with_mixed_additions(ctx, pool, bases):
    n = 1000
    want = C.expect_from_products(pool["prod"][:n])
    try:
        for cap in (4, 1):                         # chunks, two and more fold levels, odd tails
            ctx.set_msm_run_max(cap)
            for c in (5, 0):
                _check(ctx, bases[c], pool["k"][:n], want)
    finally:
        ctx.set_msm_run_max(0)
    n = 1025                                       # all scalars equal: one bucket per window holds every term
    k = np.ascontiguousarray(np.broadcast_to(pool["k"][5], (n, 4)))
    want = C.expect(pool["p"][:n], k)
    for c in WIDTHS:
        _check(ctx, bases[c], k, want)


@pytest.mark.parametrize("c", [2, 5, 11])
def test_planted_rows_and_the_off_subgroup_base(ctx, pool, c):
    import substrate_bn as bn
    n = 257
    p, k = C.planted(pool["p"][:n], pool["k"][:n], c)
    assert np.array_equal(p[C.OFF_AT], C.off_subgroup_point())
    want = C.expect(p, k)
    with bn.G2Basis(p, window=c, ctx=ctx) as b:
        _check(ctx, b, k, want)
        assert np.array_equal(ctx.g2_msm(p, k), want)
        _check(ctx, b, k[:C.OFF_AT + 1], C.expect(p[:C.OFF_AT + 1], k[:C.OFF_AT + 1]))   # the off-subgroup base last
        try:
            ctx.set_msm_run_max(4)
            _check(ctx, b, k, want)
        finally:
            ctx.set_msm_run_max(0)


@pytest.mark.parametrize("at", [6, 7, C.OFF_AT])
def test_one_term_at_an_even_and_an_odd_base_index(ctx, pool, bases, at):
    """One nonzero scalar in a prefix: a single entry per window, so in every wave that works at
    all one lane pair adds and its neighbours idle; and n = 1 itself, one pair in the grid."""
    k = np.zeros((at + 1, 4), np.uint64)
    k[at] = pool["k"][at]
    want = C.expect(pool["p"][at:at + 1], pool["k"][at:at + 1])
    for c in WIDTHS:
        _check(ctx, bases[c], k, want)
    import substrate_bn as bn
    with bn.G2Basis(pool["p"][at:at + 2], window=5, ctx=ctx) as b:
        _check(ctx, b, pool["k"][at:at + 1], want)           # n = 1 of two bases


@pytest.mark.parametrize("nbases", [1, 64, 65])
def test_table_rows_at_the_edges_of_the_build_wave(ctx, pool, nbases):
    import substrate_bn as bn
    with bn.G2Basis(pool["p"][:nbases], window=5, ctx=ctx) as b:
        assert len(b) == nbases
        _check(ctx, b, pool["k"][:nbases], C.expect_from_products(pool["prod"][:nbases]))
    # prepared from device memory
    P = _to_dev(pool["p"][:nbases])
    import torch
    torch.cuda.synchronize()
    with bn.G2Basis(P.data_ptr(), window=5, ctx=ctx, count=nbases) as b:
        assert len(b) == nbases and b.window == 5
        _check(ctx, b, pool["k"][:nbases], C.expect_from_products(pool["prod"][:nbases]))


def test_python_front_end(ctx, pool, bases):
    import substrate_bn as bn
    from substrate_bn import _native
    n = 65
    got = bn.g2_msm_basis(bases[5], pool["k"][:n])
    assert isinstance(got, bn.G2) and np.array_equal(got.img, C.expect_from_products(pool["prod"][:n]))
    assert np.array_equal(bn.g2_msm_basis(bases[5], []).img, C.zero())
    ctx.g2_msm_basis_reserve(bases[5]._handle(), NMAX)
    ctx.g2_msm_basis_reserve(bases[5]._handle(), 0)
    assert _native.g2_basis_table_bytes(NMAX, 0) == _native.g2_basis_table_bytes(NMAX, bases[0].window)


def test_lifecycle_and_refusals(ctx, pool, bases):
    from substrate_bn import BnError, Context, _native
    L, h = _native.load(), ctx.handle
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    vp = ctypes.c_void_p
    out = np.zeros(24, np.uint64)
    po, pp, pk = (vp(a.ctypes.data) for a in (out, pool["p"], pool["k"]))
    new = vp(0x1234)
    # the prepare call: refused before anything is read, *out untouched
    assert L.bn_g2_basis_prepare(h, None, 4, 5, ctypes.byref(new)) == INVALID
    assert L.bn_g2_basis_prepare(h, pp, 4, 5, None) == INVALID
    assert L.bn_g2_basis_prepare(h, pp, 0, 5, ctypes.byref(new)) == INVALID
    assert L.bn_g2_basis_prepare(h, pp, (1 << 26) + 1, 16, ctypes.byref(new)) == INVALID
    assert L.bn_g2_basis_prepare(h, pp, (2 ** 31 - 1) // 128 + 1, 2, ctypes.byref(new)) == INVALID  # nbases * W(2) over 2^31 - 1
    for c in (-1, 1, 17, 64):
        assert L.bn_g2_basis_prepare(h, pp, 4, c, ctypes.byref(new)) == INVALID
        assert L.bn_g2_basis_prepare_dev(h, pp, 4, c, ctypes.byref(new), None) == INVALID
    assert L.bn_g2_basis_prepare_dev(h, None, 4, 5, ctypes.byref(new), None) == INVALID
    assert L.bn_g2_basis_prepare_dev(h, pp, 4, 5, None, None) == INVALID
    assert new.value == 0x1234
    # the MSM call
    b5 = vp(bases[5]._handle())
    assert L.bn_g2_msm_basis(h, None, pk, 4, po) == INVALID
    assert L.bn_g2_msm_basis(h, b5, None, 4, po) == INVALID
    assert L.bn_g2_msm_basis(h, b5, pk, 4, None) == INVALID
    assert L.bn_g2_msm_basis(h, b5, pk, NMAX + 1, po) == INVALID
    assert L.bn_g2_msm_basis_dev(h, b5, pk, NMAX + 1, po, None) == INVALID
    assert L.bn_g2_msm_basis_dev(h, b5, None, 4, po, None) == INVALID
    assert L.bn_g2_msm_basis_dev(h, b5, pk, 4, None, None) == INVALID
    assert L.bn_g2_msm_basis_dev(h, None, pk, 4, po, None) == INVALID
    assert L.bn_g2_msm_basis_reserve(h, b5, NMAX + 1) == INVALID
    assert L.bn_g2_msm_basis_reserve(h, None, 4) == INVALID
    assert L.bn_g2_basis_destroy(h, None) == INVALID
    # a G1 basis handle is foreign to the G2 calls, and a G2 one to the G1 calls
    g1h = ctx.g1_basis_prepare(O.g1_mul(O.g1_one(), pool["k"][:4], NT), 5)
    assert L.bn_g2_msm_basis(h, vp(g1h), pk, 4, po) == INVALID
    assert L.bn_g2_basis_destroy(h, vp(g1h)) == INVALID
    assert L.bn_g1_msm_basis(h, b5, pk, 4, po) == INVALID
    ctx.g1_basis_destroy(g1h)
    assert not out.any()
    # a second context refuses the handle; the context that owns it goes on working
    other = Context(0)
    assert L.bn_g2_msm_basis(other.handle, b5, pk, 4, po) == INVALID
    assert L.bn_g2_basis_destroy(other.handle, b5) == INVALID
    assert L.bn_g2_msm_basis_reserve(other.handle, b5, 4) == INVALID
    other.close()
    want = C.expect_from_products(pool["prod"][:65])
    _check(ctx, bases[5], pool["k"][:65], want)
    # a destroyed handle is refused (looked up, never dereferenced)
    dead = ctx.g2_basis_prepare(pool["p"][:3], 5)
    assert ctx.g2_basis_count(dead) == 3 and ctx.g2_basis_window(dead) == 5
    ctx.g2_basis_destroy(dead)
    assert L.bn_g2_msm_basis(h, vp(dead), pk, 3, po) == INVALID
    assert L.bn_g2_basis_destroy(h, vp(dead)) == INVALID
    with pytest.raises(BnError) as e:
        ctx.g2_msm_basis_dev(dead, 0, 0, 0)
    assert e.value.code == INVALID
    # two live handles of different widths used alternately
    for _ in range(2):
        for c in (2, 0, 5):
            assert np.array_equal(ctx.g2_msm_basis(bases[c]._handle(), pool["k"][:65]), want), c
    # a multi-device context refuses; its device context works
    mctx = Context(devices=[0, 0])
    assert L.bn_g2_basis_prepare(mctx.handle, pp, 4, 5, ctypes.byref(new)) == INVALID and new.value == 0x1234
    assert L.bn_g2_basis_prepare_dev(mctx.handle, pp, 4, 5, ctypes.byref(new), None) == INVALID and new.value == 0x1234
    assert L.bn_g2_msm_basis(mctx.handle, b5, pk, 4, po) == INVALID
    assert L.bn_g2_msm_basis_dev(mctx.handle, b5, pk, 4, po, None) == INVALID
    assert L.bn_g2_msm_basis_reserve(mctx.handle, b5, 4) == INVALID
    assert L.bn_g2_basis_destroy(mctx.handle, b5) == INVALID
    sub = vp(L.bn_ctx_device(mctx.handle, 0))
    made = vp()
    assert L.bn_g2_basis_prepare(sub, pp, 65, 5, ctypes.byref(made)) == 0 and made.value
    assert L.bn_g2_msm_basis(sub, made, pk, 65, po) == 0
    assert np.array_equal(out, want)
    assert L.bn_g2_basis_destroy(sub, made) == 0
    mctx.close()


def test_a_context_frees_its_live_handles(pool):
    from substrate_bn import Context
    c = Context(0)
    h = c.g2_basis_prepare(pool["p"][:65], 5)
    assert np.array_equal(c.g2_msm_basis(h, pool["k"][:65]), C.expect_from_products(pool["prod"][:65]))
    c.close()                                      # the handle is still alive


@pytest.mark.parametrize("streams", [1, 2])
def test_sequencing_without_host_synchronization(ctx, pool, bases, streams):
    """bn_g2_msm_basis_dev, bn_pairing_batch_dev, bn_g2_msm_basis_dev, bn_g2_msm_dev,
    bn_g1_msm_basis_dev, bn_g2_msm_basis_dev with no host synchronization between them, on one
    caller stream and alternated over two: the shared G2 MSM workspace and integer buffers, and
    the header's ordering promise for the workspace-ordered _dev calls."""
    import torch
    n = 257
    dev = torch.device("cuda", 0)
    p, q, _, _ = O.random_pairs(3, seed=7104, nthreads=NT)
    h = bases[0]._handle()
    ctx.g2_msm_basis_reserve(h, n)
    m_alone = ctx.g2_msm_basis(h, pool["k"][:n])
    assert np.array_equal(m_alone, C.expect_from_products(pool["prod"][:n]))
    pb_alone = ctx.pairing_batch(p, q)
    assert np.array_equal(pb_alone, O.pairing_batch(p, q))
    half_alone = ctx.g2_msm(pool["p"][:100], pool["k"][:100])
    assert np.array_equal(half_alone, C.expect_from_products(pool["prod"][:100]))
    g1p = O.g1_mul(O.g1_one(), pool["k"][200:265], NT)
    g1h = ctx.g1_basis_prepare(g1p, 5)
    g1_alone = ctx.g1_msm_basis(g1h, pool["k"][:65])
    assert np.array_equal(g1_alone, ctx.g1_msm(g1p, pool["k"][:65]))
    P, K, P3, Q3 = _to_dev(pool["p"][:n]), _to_dev(pool["k"][:n]), _to_dev(p), _to_dev(q)
    o = [torch.full((24,), PATTERN, dtype=torch.int64, device=dev) for _ in range(4)]
    o1 = torch.full((12,), PATTERN, dtype=torch.int64, device=dev)
    o2 = torch.zeros(48, dtype=torch.int64, device=dev)
    ss = [torch.cuda.Stream(dev) for _ in range(streams)]
    s = [ss[i % streams].cuda_stream for i in range(6)]
    torch.cuda.synchronize(dev)
    ctx.g2_msm_basis_dev(h, K.data_ptr(), n, o[0].data_ptr(), s[0])
    ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, o2.data_ptr(), None, s[1])
    ctx.g2_msm_basis_dev(h, K.data_ptr(), n, o[1].data_ptr(), s[2])
    ctx.g2_msm_dev(P.data_ptr(), K.data_ptr(), 100, o[2].data_ptr(), s[3])
    ctx.g1_msm_basis_dev(g1h, K.data_ptr(), 65, o1.data_ptr(), s[4])
    ctx.g2_msm_basis_dev(bases[5]._handle(), K.data_ptr(), n, o[3].data_ptr(), s[5])
    torch.cuda.synchronize(dev)
    ctx.g1_basis_destroy(g1h)
    got = [t.cpu().numpy().view(np.uint64) for t in o]
    assert np.array_equal(got[0], m_alone) and np.array_equal(got[1], m_alone) and np.array_equal(got[3], m_alone)
    assert np.array_equal(o2.cpu().numpy().view(np.uint64), pb_alone)
    assert np.array_equal(got[2], half_alone)
    assert np.array_equal(o1.cpu().numpy().view(np.uint64), g1_alone)
