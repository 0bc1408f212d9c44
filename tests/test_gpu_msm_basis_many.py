"""A batch of scalar vectors over one fixed G1 basis at the C ABI (bn_g1_msm_basis_many,
bn_g1_msm_basis_many_dev) against the oracle, bit for bit on the 12 words of every row's
normalized image, and against bn_g1_msm_basis on the same row.  The expected value is the
oracle's alone: O.g1_mul of every term, a halving tree of O.g1_add, O.g1_normalize; a zero sum
is the (0, one, 0) image."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_basis_cases as C

pytestmark = pytest.mark.gpu
NT = C.NT
MS = [1, 2, 3, 17]
SIZES = [0, 1, 2, 63, 64, 65, 257, 1000]
WIDTHS = [2, 5, 0]
NMAX = 1000
MMAX = 17
PATTERN = 0x5a5a


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    c = Context(0)
    c.set_msm_min(0)
    return c


@pytest.fixture(scope="module")
def pool():
    """NMAX bases, MMAX rows of NMAX scalars, the oracle's product of every (row, base) and the
    expected image of every row at every size of SIZES, computed once and left unchanged."""
    p = C.g1_points(NMAX, 7101)
    _, k = O.random_scalars(MMAX * NMAX, seed=7102, lo=0)
    k = np.ascontiguousarray(k.reshape(MMAX, NMAX, 4))
    prod = O.g1_mul(np.ascontiguousarray(np.broadcast_to(p, (MMAX, NMAX, 12))).reshape(-1, 12), k.reshape(-1, 4),
                    nthreads=NT).reshape(MMAX, NMAX, 12)
    want = {n: np.stack([C.expect_from_products(prod[j, :n]) for j in range(MMAX)]) for n in SIZES}
    for a in (p, k, prod, *want.values()):
        a.setflags(write=False)
    return {"p": p, "k": k, "prod": prod, "want": want}


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


def _pattern(points):
    import torch
    return torch.full((max(points, 1) * 12,), PATTERN, dtype=torch.int64, device=torch.device("cuda", 0))


def _dev(ctx, handle, k, n, out_stride=1):
    """The whole (m * out_stride, 12) buffer of the _dev form over rows k (m, k_stride, 4),
    pre-filled with PATTERN."""
    import torch
    dev = torch.device("cuda", 0)
    m, k_stride = k.shape[0], k.shape[1]
    K = _to_dev(k) if k.size else torch.zeros(4, dtype=torch.int64, device=dev)
    out = _pattern(m * out_stride)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g1_msm_basis_many_dev(handle, K.data_ptr(), k_stride, m, n, out.data_ptr(), out_stride)
    ctx.dev_status()  # synchronizes the context's stream
    return out.cpu().numpy().view(np.uint64).reshape(-1, 12)[:m * out_stride]


def _check(ctx, basis, k, n, want, out_stride=1):
    """Both forms over rows k (m, k_stride >= n, 4): output j at row j * out_stride, the rows
    between untouched (the host mirror's zeros, the device buffer's pattern)."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    m, h = k.shape[0], basis._handle()
    host = ctx.g1_msm_basis_many(h, k, n=n, out_stride=out_stride)
    dev = _dev(ctx, h, k, n, out_stride)
    assert host.shape == dev.shape == (m * out_stride, 12)
    assert np.array_equal(host[::out_stride], want), "host form"
    assert np.array_equal(dev[::out_stride], want), "device form"
    between = np.ones(m * out_stride, bool)
    between[::out_stride] = False
    assert not host[between].any() and (dev[between] == PATTERN).all(), "the points between outputs"


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_shapes(ctx, pool, bases, n, c):
    b = bases[c]
    want = pool["want"][n]
    single = np.stack([ctx.g1_msm_basis(b._handle(), pool["k"][j, :n]) for j in range(MMAX)])
    assert np.array_equal(single, want)                    # bn_g1_msm_basis on every row
    for m in MS:
        _check(ctx, b, pool["k"][:m, :n], n, want[:m])


@pytest.mark.parametrize("c", WIDTHS)
def test_strides(ctx, pool, bases, c):
    for m, n in ((3, 65), (17, 257), (2, 0)):
        want = pool["want"][n][:m]
        _check(ctx, bases[c], pool["k"][:m, :n], n, want, out_stride=3)
        _check(ctx, bases[c], pool["k"][:m], n, want)                  # rows of the whole matrix: k_stride = NMAX
        _check(ctx, bases[c], pool["k"][:m, :n + 3], n, want, out_stride=3)


@pytest.mark.parametrize("S", [1, 2, 16])
def test_forced_launch_sets(ctx, pool, bases, S):
    """17 vectors in sets of 1, 2 and 16: the last set holds one vector."""
    try:
        ctx.set_msm_basis_many_set(S)
        for c in WIDTHS:
            for n in (65, 1000):
                _check(ctx, bases[c], pool["k"][:, :n], n, pool["want"][n])
        _check(ctx, bases[5], pool["k"][:3, :257], 257, pool["want"][257][:3], out_stride=3)
    finally:
        ctx.set_msm_basis_many_set(0)


@pytest.mark.parametrize("cap", [4, 1])
def test_run_caps_with_one_row_all_equal(ctx, pool, bases, cap):
    """Long keys and fold levels (1: three of them) in one vector only, between random rows."""
    n = 1000
    k = pool["k"][:3, :n].copy()
    k[1] = pool["k"][1, 5]
    want = pool["want"][n][:3].copy()
    want[1] = C.expect(pool["p"][:n], k[1])
    try:
        ctx.set_msm_run_max(cap)
        for c in (5, 0):
            _check(ctx, bases[c], k, n, want)
            assert np.array_equal(ctx.g1_msm_basis(bases[c]._handle(), k[1]), want[1])
        ctx.set_msm_basis_many_set(2)
        _check(ctx, bases[5], k, n, want)
        _check(ctx, bases[0], pool["k"][:, :n], n, pool["want"][n])    # 17 random rows at that cap
    finally:
        ctx.set_msm_run_max(0)
        ctx.set_msm_basis_many_set(0)
    _check(ctx, bases[0], k, n, want)                                   # the default cap


def test_zero_row_and_identical_rows(ctx, pool, bases):
    n = 257
    k = pool["k"][:4, :n].copy()
    k[1] = 0
    k[3] = k[2]
    want = pool["want"][n][:4].copy()
    want[1] = C.zero()
    want[3] = want[2]
    for c in WIDTHS:
        _check(ctx, bases[c], k, n, want)
    _check(ctx, bases[5], np.zeros((3, 65, 4), np.uint64), 65, np.stack([C.zero()] * 3))


def test_widest_window_smallest_default_set(ctx, pool):
    """c = 16 at 65 bases: 2^19 keys per vector, a default launch set of 16 vectors."""
    import substrate_bn as bn
    n = 65
    with bn.G1Basis(pool["p"][:n], window=16, ctx=ctx) as b:
        assert b.window == 16
        _check(ctx, b, pool["k"][:3, :n], n, pool["want"][n][:3])
        assert np.array_equal(ctx.g1_msm_basis(b._handle(), pool["k"][2, :n]), pool["want"][n][2])


@pytest.mark.parametrize("nbases", [1, 64, 65])
def test_small_handles(ctx, pool, nbases):
    import substrate_bn as bn
    with bn.G1Basis(pool["p"][:nbases], window=5, ctx=ctx) as b:
        _check(ctx, b, pool["k"][:3, :nbases], nbases, pool["want"][nbases][:3])
        _check(ctx, b, pool["k"][:17, :1], 1, pool["want"][1])


def test_python_front_end(ctx, pool, bases):
    import substrate_bn as bn
    n = 65
    got = bn.g1_msm_basis_many(bases[5], pool["k"][:3, :n])
    assert got.shape == (3, 12) and np.array_equal(got, pool["want"][n][:3])
    rows = [[bn.Fr(pool["k"][j, i]) for i in range(2)] for j in range(2)]
    assert np.array_equal(bn.g1_msm_basis_many(bases[5], rows), pool["want"][2][:2])
    assert bn.g1_msm_basis_many(bases[5], []).shape == (0, 12)
    ctx.g1_msm_basis_many_reserve(bases[5]._handle(), MMAX, NMAX)
    ctx.g1_msm_basis_many_reserve(bases[5]._handle(), 0, NMAX)
    ctx.g1_msm_basis_many_reserve(bases[5]._handle(), MMAX, 0)
    _check(ctx, bases[5], pool["k"][:, :NMAX], NMAX, pool["want"][NMAX])


def test_refusals(ctx, pool, bases):
    from substrate_bn import BnError, Context, _native
    L, h = _native.load(), ctx.handle
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    vp = ctypes.c_void_p
    out = np.zeros((6, 12), np.uint64)
    k = np.ascontiguousarray(pool["k"][:2, :8])
    po, pk = vp(out.ctypes.data), vp(k.ctypes.data)
    b5 = vp(bases[5]._handle())
    many, many_dev, reserve = L.bn_g1_msm_basis_many, L.bn_g1_msm_basis_many_dev, L.bn_g1_msm_basis_many_reserve
    for f, tail in ((many, ()), (many_dev, (None,))):
        assert f(h, b5, pk, 8, 2, 8, None, 1, *tail) == INVALID               # a NULL out
        assert f(h, b5, None, 8, 2, 8, po, 1, *tail) == INVALID               # a NULL k with m * n > 0
        assert f(h, b5, pk, NMAX + 1, 2, NMAX + 1, po, 1, *tail) == INVALID   # n above the handle's count
        assert f(h, b5, pk, 7, 2, 8, po, 1, *tail) == INVALID                 # k_stride < n
        assert f(h, b5, pk, 8, 2, 8, po, 0, *tail) == INVALID                 # out_stride == 0
        assert f(h, b5, pk, 8, (1 << 26) + 1, 8, po, 1, *tail) == INVALID     # m above 2^26
        assert f(h, None, pk, 8, 2, 8, po, 1, *tail) == INVALID               # no handle
        assert f(h, b5, pk, 8, 0, 8, po, 1, *tail) == 0                       # m == 0: BN_OK, nothing touched
        assert f(h, b5, None, 8, 0, 8, po, 1, *tail) == 0
    assert reserve(h, None, 2, 8) == INVALID and reserve(h, b5, 2, NMAX + 1) == INVALID
    assert reserve(h, b5, (1 << 26) + 1, 8) == INVALID
    assert L.bn_set_msm_basis_many_set(h, (1 << 26) + 1) == INVALID
    assert not out.any()
    # n == 0 with a NULL k: the zero images
    assert many(h, b5, None, 0, 2, 0, po, 3) == 0
    assert np.array_equal(out[0], C.zero()) and np.array_equal(out[3], C.zero()) and not out[1:3].any() and not out[4:].any()
    out[:] = 0
    # a second context refuses the handle; a destroyed handle is refused
    other = Context(0)
    assert many(other.handle, b5, pk, 8, 2, 8, po, 1) == INVALID
    assert reserve(other.handle, b5, 2, 8) == INVALID
    other.close()
    dead = ctx.g1_basis_prepare(pool["p"][:8], 5)
    ctx.g1_basis_destroy(dead)
    assert many(h, vp(dead), pk, 8, 2, 8, po, 1) == INVALID
    with pytest.raises(BnError) as e:
        ctx.g1_msm_basis_many_dev(dead, 0, 0, 1, 0, 0)
    assert e.value.code == INVALID
    assert not out.any()
    # a multi-device context refuses; its device context works; the setting reaches its devices
    mctx = Context(devices=[0, 0])
    assert many(mctx.handle, b5, pk, 8, 2, 8, po, 1) == INVALID
    assert many_dev(mctx.handle, b5, pk, 8, 2, 8, po, 1, None) == INVALID
    assert reserve(mctx.handle, b5, 2, 8) == INVALID
    assert not out.any()
    assert L.bn_set_msm_basis_many_set(mctx.handle, 1) == 0
    sub = vp(L.bn_ctx_device(mctx.handle, 0))
    made = vp()
    pp = vp(pool["p"].ctypes.data)
    assert L.bn_g1_basis_prepare(sub, pp, 65, 5, ctypes.byref(made)) == 0 and made.value
    assert many(sub, made, pk, 8, 2, 8, po, 3) == 0
    assert np.array_equal(out[0], C.expect_from_products(pool["prod"][0, :8]))
    assert np.array_equal(out[3], C.expect_from_products(pool["prod"][1, :8]))
    assert L.bn_g1_basis_destroy(sub, made) == 0
    mctx.close()
    # the context that owns the handle goes on working
    _check(ctx, bases[5], pool["k"][:2, :65], 65, pool["want"][65][:2])


def test_sequencing_on_one_stream(ctx, pool, bases):
    """bn_g1_msm_basis_many_dev, bn_g1_msm_basis_dev, bn_g1_msm_basis_many_dev on one caller
    stream with no host synchronization between them: the two forms reuse one workspace."""
    import torch
    dev = torch.device("cuda", 0)
    n, m = 257, 3
    h = bases[0]._handle()
    ctx.g1_msm_basis_many_reserve(h, m, n)
    K = _to_dev(pool["k"][:m])                              # rows of the whole matrix: k_stride = NMAX
    o0, o1, o2 = _pattern(m), _pattern(1), _pattern(m * 2)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ctx.g1_msm_basis_many_dev(h, K.data_ptr(), NMAX, m, n, o0.data_ptr(), 1, s.cuda_stream)
    ctx.g1_msm_basis_dev(h, K.data_ptr() + 2 * NMAX * 32, 1000, o1.data_ptr(), s.cuda_stream)
    ctx.g1_msm_basis_many_dev(bases[5]._handle(), K.data_ptr(), NMAX, m, 65, o2.data_ptr(), 2, s.cuda_stream)
    torch.cuda.synchronize(dev)
    got = [t.cpu().numpy().view(np.uint64).reshape(-1, 12) for t in (o0, o1, o2)]
    assert np.array_equal(got[0], pool["want"][n][:m])
    assert np.array_equal(got[1][0], pool["want"][1000][2])
    assert np.array_equal(got[2][::2], pool["want"][65][:m]) and (got[2][1::2] == PATTERN).all()
