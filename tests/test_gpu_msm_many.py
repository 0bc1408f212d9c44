"""Many small G1 MSMs over fresh bases at the C ABI (bn_g1_msm_many and its _dev form)
against the oracle, bit for bit on the 12 words of every output.  The expected rows are the
oracle's alone (tests/msm_many_cases.py): O.g1_mul of every term, a halving tree of O.g1_add
per segment, O.g1_normalize; a zero sum and an empty segment are the (0, one, 0) image.
Every case runs with 1, 2 and 16 terms per unit forced and with the automatic choice at
each of the widths 2, 4 and 8, with launch sets of 64 terms forced, by the host form and the
device-pointer form; all must give the same bytes.  The largest case is 257 segments of 17
terms; the longest segment has 1,025."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_g2_cases as C2
from tests import msm_many_cases as M

pytestmark = pytest.mark.gpu
MS = [0, 1, 2, 63, 65, 257]
LENS = [1, 2, 17]
RAGGED = [0, 1, 15, 16, 17, 65]
LONG = 1025
NPOOL = 257 * 17
FILL = 0x5a5a
INVALID = 1
CAP = 1 << 26


def _defaults(c):
    c.set_msm_many_window(0)
    c.set_msm_many_unit(0)
    c.set_msm_many_max(0)
    c.set_msm_many_chunk(0)


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    c = Context(0)
    yield c
    _defaults(c)


@pytest.fixture(scope="module")
def pool():
    """NPOOL points and scalars, the oracle's product of every term and, from those, the
    expected rows of every shape the tests use, computed once."""
    p = M.g1_points(NPOOL, 8401)
    assert not np.array_equal(p[0, 8:12], O.canon_to_mont_array([1]).reshape(4))  # Jacobian, z != one
    _, k = O.random_scalars(NPOOL, seed=8402, lo=0)
    prod = M.products(p, k)
    want = {L: M.expect_from_products(prod[:257 * L], M.offsets_of([L] * 257)) for L in LENS}
    want["ragged"] = M.expect_from_products(prod[:sum(RAGGED)], M.offsets_of(RAGGED))
    want["long"] = M.expect_from_products(prod[:LONG], M.offsets_of([LONG]))
    for a in [p, k, prod] + list(want.values()):
        a.setflags(write=False)
    return {"p": p, "k": k, "want": want}


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.zeros(12, dtype=torch.int64, device=torch.device("cuda", 0))
    return torch.from_numpy(a.view(np.int64).reshape(-1).copy()).to(torch.device("cuda", 0))


def _dev(ctx, p, k, off, stride=1, stream=None):
    """the (m * stride, 12) buffer, pre-filled with FILL, after the _dev form"""
    import torch
    dev = torch.device("cuda", 0)
    m = len(off) - 1
    P, K = _to_dev(p), _to_dev(k)
    out = torch.full((max(m * stride, 1) * 12,), FILL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), off, out.data_ptr(), stride, stream)
    ctx.dev_status(stream)  # synchronizes
    return out.cpu().numpy().view(np.uint64).reshape(-1, 12)[:m * stride]


def _all_ways(ctx, p, k, off, max_terms=0):
    """{name: (m, 12)} of the same call at every width with every unit setting, with launch
    sets of 64 terms, and by the _dev form (max_terms: bn_set_msm_many_max for all of them)"""
    got = {}
    try:
        ctx.set_msm_many_max(max_terms)
        for c in (2, 4, 8):
            ctx.set_msm_many_window(c)
            for unit in (1, 2, 16, 0):
                ctx.set_msm_many_unit(unit)
                got["c %d, unit %d" % (c, unit)] = ctx.g1_msm_many(p, k, off)
            got["dev, c %d, unit 0" % c] = _dev(ctx, p, k, off)
        ctx.set_msm_many_window(0)
        ctx.set_msm_many_chunk(64)
        got["chunk 64, unit 0"] = ctx.g1_msm_many(p, k, off)
        ctx.set_msm_many_unit(2)
        got["chunk 64, unit 2"] = ctx.g1_msm_many(p, k, off)
        got["dev, chunk 64, unit 2"] = _dev(ctx, p, k, off)
    finally:
        _defaults(ctx)
    return got


def _check(ctx, p, k, off, want, max_terms=0):
    for name, out in _all_ways(ctx, p, k, off, max_terms).items():
        assert out.shape == want.shape, name
        bad = [j for j in range(want.shape[0]) if not np.array_equal(out[j], want[j])]
        assert not bad, "%s: rows %s of %d differ" % (name, bad[:8], want.shape[0])


def _same_as_single(ctx, p, k, off, want):
    m = len(off) - 1
    for j in sorted({0, m // 2, m - 1} & set(range(m))):   # the image bn_g1_msm returns for the same slice
        lo, hi = int(off[j]), int(off[j + 1])
        assert np.array_equal(ctx.g1_msm(p[lo:hi], k[lo:hi]), want[j]), j


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("length", LENS)
def test_uniform(ctx, pool, length, m):
    n = m * length
    p, k, off = pool["p"][:n], pool["k"][:n], M.offsets_of([length] * m)
    want = pool["want"][length][:m]
    if m == 0:   # nothing is called for; the raw library returns BN_OK and touches nothing (test_argument_checks)
        assert ctx.g1_msm_many(p, k, off).shape == (0, 12)
        return
    _check(ctx, p, k, off, want)
    _same_as_single(ctx, p, k, off, want)


def test_ragged(ctx, pool):
    n = sum(RAGGED)
    p, k, off = pool["p"][:n], pool["k"][:n], M.offsets_of(RAGGED)
    want = pool["want"]["ragged"]
    assert np.array_equal(want[0], M.zero())
    _check(ctx, p, k, off, want)
    _same_as_single(ctx, p, k, off, want)


def test_only_empty_segments(ctx):
    want = np.ascontiguousarray(np.broadcast_to(M.zero(), (65, 12)))
    _check(ctx, np.zeros((0, 12), np.uint64), np.zeros((0, 4), np.uint64), M.offsets_of([0] * 65), want)


def test_one_long_segment_packed_and_alone(ctx, pool):
    p, k, off = pool["p"][:LONG], pool["k"][:LONG], M.offsets_of([LONG])
    want = pool["want"]["long"]
    try:
        _check(ctx, p, k, off, want, 4096)         # packed: units of ceil(1025 / 64) = 17 terms
        ctx.set_msm_many_max(1024)                 # alone: bn_g1_msm's path
        assert np.array_equal(ctx.g1_msm_many(p, k, off), want)
        assert np.array_equal(_dev(ctx, p, k, off), want)
        # alone between packed neighbours, at a stride
        off3 = M.offsets_of([3, LONG - 5, 2])
        want3 = M.expect_from_products(M.products(p, k), off3)
        ctx.set_msm_many_max(16)
        assert np.array_equal(ctx.g1_msm_many(p, k, off3), want3)
        got = _dev(ctx, p, k, off3, 2)
        assert np.array_equal(got[::2], want3) and (got[1::2] == FILL).all()
    finally:
        _defaults(ctx)
    assert np.array_equal(ctx.g1_msm(p, k), want[0])


@pytest.mark.parametrize("c", [2, 4, 8])
def test_planted_rows(ctx, pool, c):
    for zero_form in (0, 1):
        p, vals, off = M.planted(pool["p"][:5], c, zero_form)
        k = M.fr(vals)
        want = M.expect(p, k, off)
        assert np.array_equal(want[0], M.zero()) and np.array_equal(want[2], M.zero())
        try:
            ctx.set_msm_many_window(c)
            for unit in (1, 2, 16):
                ctx.set_msm_many_unit(unit)
                got = ctx.g1_msm_many(p, k, off)
                bad = [j for j in range(len(want)) if not np.array_equal(got[j], want[j])]
                assert not bad, (zero_form, unit, bad)
            assert np.array_equal(_dev(ctx, p, k, off), want)
        finally:
            _defaults(ctx)


def test_normalized_points_give_the_same_bytes(ctx, pool):
    n = 65 * 2
    off = M.offsets_of([2] * 65)
    assert np.array_equal(ctx.g1_msm_many(O.g1_normalize(pool["p"][:n]), pool["k"][:n], off), pool["want"][2][:65])


def test_stride(ctx, pool):
    from substrate_bn import _native
    m, length, stride = 65, 2, 3
    n = m * length
    p, k, off = np.array(pool["p"][:n]), np.array(pool["k"][:n]), M.offsets_of([length] * m)
    want = np.full((m * stride, 12), FILL, np.uint64)
    want[::stride] = pool["want"][length][:m]
    host = np.full((m * stride, 12), FILL, np.uint64)
    vp = ctypes.c_void_p
    rc = _native.load().bn_g1_msm_many(ctx.handle, vp(p.ctypes.data), vp(k.ctypes.data), vp(off.ctypes.data), m,
                                       vp(host.ctypes.data), stride)
    assert rc == 0
    assert np.array_equal(host, want)             # rows 3 j hold the results, every other word is untouched
    assert np.array_equal(_dev(ctx, p, k, off, stride), want)
    py = ctx.g1_msm_many(p, k, off, out_stride=stride)
    assert np.array_equal(py[::stride], pool["want"][length][:m]) and not py.reshape(m, stride, 12)[:, 1:].any()


def test_argument_checks(ctx, pool):
    from substrate_bn import BnError, Context, _native
    L, hc = _native.load(), ctx.handle
    vp = ctypes.c_void_p
    p, k = np.array(pool["p"][:4]), np.array(pool["k"][:4])
    out = np.full((4, 12), FILL, np.uint64)
    pp, pk, po = vp(p.ctypes.data), vp(k.ctypes.data), vp(out.ctypes.data)

    def offs(*v):
        a = np.array(v, np.uintp)
        return a, vp(a.ctypes.data)

    good, pgood = offs(0, 2, 4)
    cases = [(pp, pk, offs(0, 3, 2, 4), 3, po, 1),       # decreasing
             (pp, pk, offs(1, 2, 4), 2, po, 1),          # offsets[0] != 0
             (pp, pk, (None, None), 2, po, 1),           # NULL offsets
             (pp, pk, (good, pgood), 2, None, 1),        # NULL out
             (None, pk, (good, pgood), 2, po, 1),        # NULL p with n > 0
             (pp, None, (good, pgood), 2, po, 1),        # NULL k with n > 0
             (pp, pk, (good, pgood), 2, po, 0),          # out_stride 0
             (pp, pk, offs(0, CAP + 1), 1, po, 1),       # n above 2^26: refused before any buffer is read
             (pp, pk, (good, pgood), CAP + 1, po, 1)]    # m above 2^26: refused before offsets is read
    for a, b, (_, o), m, d, stride in cases:
        assert L.bn_g1_msm_many(hc, a, b, o, m, d, stride) == INVALID
        assert L.bn_g1_msm_many_dev(hc, a, b, o, m, d, stride, None) == INVALID
    assert L.bn_g1_msm_many(hc, None, None, None, 0, None, 1) == 0              # m == 0: nothing is touched
    assert L.bn_g1_msm_many_dev(hc, None, None, None, 0, None, 1, None) == 0
    z, pz = offs(0, 0, 0)
    assert L.bn_g1_msm_many(hc, None, None, pz, 2, po, 1) == 0                  # n == 0: p and k may be NULL
    assert np.array_equal(out[:2], np.stack([M.zero()] * 2)) and (out[2:] == FILL).all()
    out[:] = FILL
    for setter, bad in ((ctx.set_msm_many_window, (1, 9, -1, 16)), (ctx.set_msm_many_unit, (-1, 65, 128)),
                        (ctx.set_msm_many_max, (4097, 1 << 20)), (ctx.set_msm_many_chunk, (CAP + 1,))):
        for v in bad:
            with pytest.raises(BnError) as e:
                setter(v)
            assert e.value.code == INVALID
    with pytest.raises(BnError) as e:
        ctx.g1_msm_many_reserve(CAP + 1, 1)
    assert e.value.code == INVALID
    ctx.g1_msm_many_reserve(1 << 12, 1 << 8)
    # a multi-device context refuses, its device contexts work
    mctx = Context(devices=[0, 0])
    assert L.bn_g1_msm_many(mctx.handle, pp, pk, pgood, 2, po, 1) == INVALID
    assert L.bn_g1_msm_many_dev(mctx.handle, pp, pk, pgood, 2, po, 1, None) == INVALID
    assert (out == FILL).all()
    want = M.expect(p, k, good)
    assert np.array_equal(mctx.device(0).g1_msm_many(p, k, good), want)
    mctx.close()
    # the context stays usable, at its previous settings
    assert np.array_equal(ctx.g1_msm_many(p, k, good), want)


def test_sequencing_with_prepared_pairing_products(ctx, pool):
    """On one caller stream with no host synchronization: the MSMs written into every second
    slot of the products' p array, the two-term pairing products over two prepared G2 points,
    the MSMs again."""
    import torch
    dev = torch.device("cuda", 0)
    m, lengths = 3, [2, 5, 3]
    n = sum(lengths)
    p, k, off = pool["p"][:n], pool["k"][:n], M.offsets_of(lengths)
    sums = M.expect(p, k, off)
    g1 = M.g1_points(m, 8404)
    Q = C2.g2_points(2, 8405)
    pairs = np.zeros((2 * m, 12), np.uint64)
    pairs[1::2] = g1
    want_p = pairs.copy()
    want_p[0::2] = sums
    qidx = np.tile(np.array([0, 1], np.uint32), m)
    poff = np.arange(0, 2 * m + 1, 2).astype(np.uintp)
    want_gt = np.stack([O.pairing_batch(want_p[2 * j:2 * j + 2], Q) for j in range(m)])
    g2h = ctx.g2_prepare(Q)
    P, K, PAIRS = _to_dev(p), _to_dev(k), _to_dev(pairs)
    gt = torch.zeros(m * 48, dtype=torch.int64, device=dev)
    again = torch.zeros(m * 12, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    try:
        ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), off, PAIRS.data_ptr(), 2, s.cuda_stream)
        ctx.pairing_batch_prepared_many_dev(PAIRS.data_ptr(), None, g2h, qidx, poff, gt.data_ptr(), s.cuda_stream)
        ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), off, again.data_ptr(), 1, s.cuda_stream)
        torch.cuda.synchronize(dev)
        ctx.dev_status()
        assert np.array_equal(PAIRS.cpu().numpy().view(np.uint64).reshape(-1, 12), want_p)
        assert np.array_equal(again.cpu().numpy().view(np.uint64).reshape(-1, 12), sums)
        assert np.array_equal(gt.cpu().numpy().view(np.uint64).reshape(-1, 48), want_gt)
    finally:
        ctx.g2_prepared_destroy(g2h)
