"""G1 MSMs over prepared bases at the C ABI (bn_g1_bases_prepare, bn_g1_msm_prepared_many
and their _dev forms) against the oracle, bit for bit on the 12 words of every output.  The
expected rows are the oracle's alone (tests/msm_prepared_cases.py): O.g1_mul of every term,
a halving tree of O.g1_add per row, O.g1_normalize; a zero sum is the (0, one, 0) image.
Every case runs with 1, 2 and 64 lanes per output forced and with the automatic choice, by
the host form and the device-pointer form; all must give the same bytes.  The largest case
is 257 rows of 17 terms."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_g2_cases as C2
from tests import msm_prepared_cases as C

pytestmark = pytest.mark.gpu
NT = 16
KMAX, MMAX = 17, 257
KS = [1, 2, 17]
MS = [0, 1, 2, 63, 65, 257]
FILL = 0x5a5a
INVALID = 1
CAP = 1 << 26
DEFAULT_C = 10


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    c = Context(0)
    yield c
    c.set_msm_prepared_lanes(0)


@pytest.fixture(scope="module")
def pool():
    """KMAX bases, MMAX rows of KMAX scalars and the oracle's products, computed once."""
    bases = C.g1_points(KMAX, 8201)
    assert not np.array_equal(bases[0, 8:12], O.canon_to_mont_array([1]).reshape(4))  # Jacobian, z != one
    _, k = O.random_scalars(MMAX * KMAX, seed=8202, lo=0)
    k = k.reshape(MMAX, KMAX, 4)
    prod = C.products(bases, k)
    want = {kk: C.expect_from_products(prod[:, :kk]) for kk in KS + [3]}
    for a in [bases, k, prod] + list(want.values()):
        a.setflags(write=False)
    return {"bases": bases, "k": k, "want": want}


@pytest.fixture(scope="module")
def handles(ctx, pool):
    """one handle per k at the default width"""
    hs = {k: ctx.g1_bases_prepare(pool["bases"][:k]) for k in KS}
    for k, h in hs.items():
        assert ctx.g1_prepared_count(h) == k and ctx.g1_prepared_window(h) == DEFAULT_C
    yield hs
    for h in hs.values():
        ctx.g1_prepared_destroy(h)


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.zeros(12, dtype=torch.int64, device=torch.device("cuda", 0))
    return torch.from_numpy(a.view(np.int64).reshape(-1).copy()).to(torch.device("cuda", 0))


def _dev(ctx, h, scal, stride=1, stream=None):
    """the (m * stride, 12) buffer, pre-filled with FILL, after the _dev form"""
    import torch
    dev = torch.device("cuda", 0)
    m = scal.shape[0]
    K = _to_dev(scal)
    out = torch.full((max(m * stride, 1) * 12,), FILL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g1_msm_prepared_many_dev(h, K.data_ptr(), m, out.data_ptr(), stride, stream)
    ctx.dev_status(stream)  # synchronizes
    return out.cpu().numpy().view(np.uint64).reshape(-1, 12)[:m * stride]


def _all_ways(ctx, h, scal):
    """{name: (m, 12)} of the same call with 1, 2, 64 and automatic lanes, and the _dev form"""
    got = {}
    try:
        for lanes in (1, 2, 64, 0):
            ctx.set_msm_prepared_lanes(lanes)
            got["lanes %d" % lanes] = ctx.g1_msm_prepared_many(h, scal)
            if lanes in (2, 0):
                got["dev, lanes %d" % lanes] = _dev(ctx, h, scal)
    finally:
        ctx.set_msm_prepared_lanes(0)
    return got


def _check(ctx, h, scal, want):
    for name, out in _all_ways(ctx, h, scal).items():
        assert out.shape == want.shape, name
        bad = [j for j in range(want.shape[0]) if not np.array_equal(out[j], want[j])]
        assert not bad, "%s: rows %s of %d differ" % (name, bad[:8], want.shape[0])


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
def test_sizes(ctx, pool, handles, k, m):
    scal = np.ascontiguousarray(pool["k"][:m, :k])
    _check(ctx, handles[k], scal, pool["want"][k][:m])
    for j in sorted({0, m // 2, m - 1} & set(range(m))):   # the image bn_g1_msm returns for the same row
        assert np.array_equal(ctx.g1_msm(pool["bases"][:k], scal[j]), pool["want"][k][j]), j


@pytest.mark.parametrize("c", [2, 5, 13])
def test_window_widths(ctx, pool, c):
    h = ctx.g1_bases_prepare(pool["bases"][:3], c)
    try:
        assert ctx.g1_prepared_window(h) == c and ctx.g1_prepared_count(h) == 3
        _check(ctx, h, np.ascontiguousarray(pool["k"][:65, :3]), pool["want"][3][:65])
    finally:
        ctx.g1_prepared_destroy(h)


@pytest.mark.parametrize("c", [5, 0])
def test_planted_rows(ctx, pool, c):
    scal = C.planted_scalars(c or DEFAULT_C, 64, seed=8203)
    for zero_form in (0, 1):
        bases = C.planted_bases(pool["bases"], zero_form)
        want = C.expect(bases, scal)
        assert np.array_equal(want[0], C.zero()) and np.array_equal(want[2], C.zero())
        h = ctx.g1_bases_prepare(bases, c)
        try:
            _check(ctx, h, scal, want)
        finally:
            ctx.g1_prepared_destroy(h)


def test_equal_rows_and_the_all_zero_matrix(ctx, pool, handles):
    m = 130
    same = np.ascontiguousarray(np.broadcast_to(pool["k"][7, :17], (m, 17, 4)))   # every lane gathers the same entries
    _check(ctx, handles[17], same, np.ascontiguousarray(np.broadcast_to(pool["want"][17][7], (m, 12))))
    _check(ctx, handles[17], np.zeros((m, 17, 4), np.uint64), np.ascontiguousarray(np.broadcast_to(C.zero(), (m, 12))))


def test_normalized_bases_give_the_same_bytes(ctx, pool):
    h = ctx.g1_bases_prepare(O.g1_normalize(pool["bases"][:3]))
    try:
        _check(ctx, h, np.ascontiguousarray(pool["k"][:65, :3]), pool["want"][3][:65])
    finally:
        ctx.g1_prepared_destroy(h)


def test_stride(ctx, pool, handles):
    from substrate_bn import _native
    m, k, stride = 65, 2, 4
    scal = np.ascontiguousarray(pool["k"][:m, :k])
    want = np.full((m * stride, 12), FILL, np.uint64)
    want[::stride] = pool["want"][k][:m]
    host = np.full((m * stride, 12), FILL, np.uint64)
    vp = ctypes.c_void_p
    rc = _native.load().bn_g1_msm_prepared_many(ctx.handle, handles[k], vp(scal.ctypes.data), m, vp(host.ctypes.data),
                                                stride)
    assert rc == 0
    assert np.array_equal(host, want)             # rows 4 j hold the results, every other word is untouched
    assert np.array_equal(_dev(ctx, handles[k], scal, stride), want)
    py = ctx.g1_msm_prepared_many(handles[k], scal, out_stride=stride)
    assert np.array_equal(py[::stride], pool["want"][k][:m]) and not py.reshape(m, stride, 12)[:, 1:].any()


def test_handle_lifecycle(ctx, pool, handles):
    from substrate_bn import BnError, Context, _native
    # two handles with different k and c, used alternately
    h5 = ctx.g1_bases_prepare(pool["bases"][:2], 5)
    s2, s17 = np.ascontiguousarray(pool["k"][:9, :2]), np.ascontiguousarray(pool["k"][:9, :17])
    for _ in range(2):
        assert np.array_equal(ctx.g1_msm_prepared_many(h5, s2), pool["want"][2][:9])
        assert np.array_equal(ctx.g1_msm_prepared_many(handles[17], s17), pool["want"][17][:9])
    # destroyed, then used or destroyed again
    # (through the raw library: the mirror would ask the freed handle for its count)
    ctx.g1_prepared_destroy(h5)
    L, vp = _native.load(), ctypes.c_void_p
    out = np.full((9, 12), FILL, np.uint64)
    assert L.bn_g1_msm_prepared_many(ctx.handle, h5, vp(s2.ctypes.data), 9, vp(out.ctypes.data), 1) == INVALID
    assert L.bn_g1_msm_prepared_many_dev(ctx.handle, h5, None, 9, None, 1, None) == INVALID
    assert L.bn_g1_prepared_destroy(ctx.handle, h5) == INVALID
    assert (out == FILL).all()
    # a handle of another context; that context is then destroyed with its handle alive
    other = Context(0)
    ho = other.g1_bases_prepare(pool["bases"][:2])
    assert np.array_equal(other.g1_msm_prepared_many(ho, s2), pool["want"][2][:9])
    for c, h in ((ctx, ho), (other, handles[2])):
        with pytest.raises(BnError) as e:
            c.g1_msm_prepared_many(h, s2)
        assert e.value.code == INVALID
        with pytest.raises(BnError) as e:
            c.g1_prepared_destroy(h)
        assert e.value.code == INVALID
    other.close()
    # a multi-device context refuses, its device contexts work
    mctx = Context(devices=[0, 0])
    with pytest.raises(BnError) as e:
        mctx.g1_bases_prepare(pool["bases"][:2])
    assert e.value.code == INVALID
    with pytest.raises(BnError) as e:
        mctx.g1_msm_prepared_many_dev(handles[2], 0, 0, 0)
    assert e.value.code == INVALID
    sub = mctx.device(0)
    hs = sub.g1_bases_prepare(pool["bases"][:2])
    assert np.array_equal(sub.g1_msm_prepared_many(hs, s2), pool["want"][2][:9])
    mctx.close()                                  # with hs alive
    assert np.array_equal(ctx.g1_msm_prepared_many(handles[2], s2), pool["want"][2][:9])


def test_argument_checks(ctx, pool, handles):
    from substrate_bn import BnError, _native
    L, hc = _native.load(), ctx.handle
    vp = ctypes.c_void_p
    bases = np.array(pool["bases"][:2])
    scal = np.ascontiguousarray(pool["k"][:4, :2])
    out = np.full((4, 12), FILL, np.uint64)
    pb, pk, po = vp(bases.ctypes.data), vp(scal.ctypes.data), vp(out.ctypes.data)
    h = ctypes.c_void_p(0x77)
    for args in ((None, 2, 8, ctypes.byref(h)), (pb, 2, 8, None), (pb, 0, 8, ctypes.byref(h)),
                 (pb, 2, 1, ctypes.byref(h)), (pb, 2, 17, ctypes.byref(h)), (pb, 2, -1, ctypes.byref(h)),
                 (pb, 1 << 40, 8, ctypes.byref(h))):
        assert L.bn_g1_bases_prepare(hc, *args) == INVALID, args[1:3]
        assert L.bn_g1_bases_prepare_dev(hc, *args, None) == INVALID, args[1:3]
    assert h.value == 0x77                         # *out untouched
    good = handles[2]
    assert L.bn_g1_msm_prepared_many(hc, good, None, 4, po, 1) == INVALID
    assert L.bn_g1_msm_prepared_many(hc, good, pk, 4, None, 1) == INVALID
    assert L.bn_g1_msm_prepared_many(hc, None, pk, 4, po, 1) == INVALID
    assert L.bn_g1_msm_prepared_many(hc, good, pk, 4, po, 0) == INVALID
    assert L.bn_g1_msm_prepared_many(hc, good, pk, CAP + 1, po, 1) == INVALID     # refused before any buffer is read
    assert L.bn_g1_msm_prepared_many_dev(hc, good, None, 4, None, 1, None) == INVALID
    assert L.bn_g1_msm_prepared_many_dev(hc, good, pk, 4, po, 0, None) == INVALID
    assert L.bn_g1_msm_prepared_many_dev(hc, good, pk, CAP + 1, po, 1, None) == INVALID
    assert L.bn_g1_msm_prepared_many(hc, good, None, 0, None, 1) == 0             # m == 0: nothing is touched
    assert L.bn_g1_msm_prepared_many_dev(hc, good, None, 0, None, 1, None) == 0
    assert (out == FILL).all()
    for lanes in (3, 128, -1, 65):
        with pytest.raises(BnError) as e:
            ctx.set_msm_prepared_lanes(lanes)
        assert e.value.code == INVALID
    # the context stays usable, at its previous settings
    assert np.array_equal(ctx.g1_msm_prepared_many(good, scal), pool["want"][2][:4])


def test_sequencing_with_prepared_pairing_products(ctx, pool):
    """On one caller stream with no host synchronization: prepare_dev, the MSMs written at
    stride 4 into the products' p array, the pairing products over it, the MSMs again."""
    import torch
    dev = torch.device("cuda", 0)
    m, k = 3, 5
    bases = np.array(pool["bases"][:k])
    scal = np.ascontiguousarray(pool["k"][:m, :k])
    vk_x = C.expect(bases, scal)
    g1 = C.g1_points(3 * m, 8204)
    Q = C2.g2_points(4, 8205)                       # three prepared points and one that stays fresh
    p = np.zeros((4 * m, 12), np.uint64)
    p[1::4], p[2::4], p[3::4] = g1[0::3], g1[1::3], g1[2::3]
    want_p = p.copy()
    want_p[0::4] = vk_x
    qidx = np.tile(np.array([0, 1, 0xFFFFFFFF, 2], np.uint32), m)
    off = np.arange(0, 4 * m + 1, 4).astype(np.uintp)
    qfull = np.stack([Q[0], Q[1], Q[3], Q[2]] * m)
    want_gt = np.stack([O.pairing_batch(want_p[4 * j:4 * j + 4], qfull[4 * j:4 * j + 4]) for j in range(m)])
    g2h = ctx.g2_prepare(Q[:3])
    B, K, P = _to_dev(bases), _to_dev(scal), _to_dev(p)
    Qf = _to_dev(np.stack([Q[3]] * m))
    gt = torch.zeros(m * 48, dtype=torch.int64, device=dev)
    again = torch.zeros(m * 12, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    h = ctx.g1_bases_prepare_dev(B.data_ptr(), k, 0, s.cuda_stream)
    try:
        ctx.g1_msm_prepared_many_dev(h, K.data_ptr(), m, P.data_ptr(), 4, s.cuda_stream)
        ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qf.data_ptr(), g2h, qidx, off, gt.data_ptr(), s.cuda_stream)
        ctx.g1_msm_prepared_many_dev(h, K.data_ptr(), m, again.data_ptr(), 1, s.cuda_stream)
        torch.cuda.synchronize(dev)
        ctx.dev_status()
        assert np.array_equal(P.cpu().numpy().view(np.uint64).reshape(-1, 12), want_p)
        assert np.array_equal(again.cpu().numpy().view(np.uint64).reshape(-1, 12), vk_x)
        assert np.array_equal(gt.cpu().numpy().view(np.uint64).reshape(-1, 48), want_gt)
    finally:
        ctx.g1_prepared_destroy(h)
        ctx.g2_prepared_destroy(g2h)
