"""Batched pairing products at the C ABI (bn_pairing_batch_many, bn_pairing_batch_many_dev)
against the oracle: row j is O.pairing_batch of the pairs offsets[j] <= i < offsets[j + 1],
bit for bit on its 48 words.  No tolerance is involved.

The first group runs the packed kernel (k_miller_products) at every product size
(bn_set_products_min(0)): sizes mixed inside one wave, product counts at the wave and
block edges, zero points, Jacobian / affine / structured edge operands.  The second group
covers the three final-exponentiation paths behind it, chunking, the routing of long and
of few products, the device-pointer form, the refusals and the sharded form."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E

pytestmark = pytest.mark.gpu
NT = 16
NPOOL = 600
LANE_MAX = 64  # kProductLaneMax: the packed kernel's largest product
ONE = np.zeros(48, np.uint64)
ONE[:4] = O.canon_to_mont_array([1]).reshape(4)


@pytest.fixture(scope="module")
def ctx():
    """The packed path at every size."""
    from substrate_bn import Context
    c = Context(0)
    c.set_products_min(0)
    return c


@pytest.fixture()
def own_ctx():
    """A context of the test's own, for the tests that turn knobs: the shared one keeps its settings."""
    from substrate_bn import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    p, q, _, _ = O.random_pairs(NPOOL, seed=8101, nthreads=NT)
    assert not np.array_equal(p[0, 8:12], ONE[:4])  # Jacobian, z != one
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    return off


def expect(p, q, off):
    """The oracle's pairing_batch of every product, computed once per input."""
    out = np.zeros((len(off) - 1, 48), np.uint64)
    for j in range(len(off) - 1):
        lo, hi = int(off[j]), int(off[j + 1])
        out[j] = O.pairing_batch(p[lo:hi], q[lo:hi], nthreads=NT if hi - lo > 16 else None)
    return out


def check(got, want, what=""):
    assert got.shape == want.shape
    bad = [j for j in range(want.shape[0]) if not np.array_equal(got[j], want[j])]
    assert not bad, "%s: products %s of %d differ" % (what, bad[:8], want.shape[0])


# ---------------------------------------------------------------- 1. the packed kernel
def test_sizes_mixed_inside_one_wave(ctx, pool):
    sizes = ([0, 1, 2, 5, 0, 3, 1, 64, 1] * 5)[:40]
    off = offsets_of(sizes)
    n = int(off[-1])
    assert n <= NPOOL and max(sizes) == LANE_MAX
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    assert all(np.array_equal(want[j], ONE) for j, s in enumerate(sizes) if s == 0)
    check(ctx.pairing_batch_many(p, q, off), want)


@pytest.fixture(scope="module")
def edge_counts(pool):
    """257 products of one or two terms and the oracle's rows; fewer products are a prefix."""
    sizes = [1 + (j % 2) for j in range(257)]
    off = offsets_of(sizes)
    n = int(off[-1])
    return off, expect(pool[0][:n], pool[1][:n], off)


@pytest.mark.parametrize("m", [31, 32, 33, 255, 256, 257])
def test_product_counts_at_wave_and_block_edges(ctx, pool, edge_counts, m):
    off, want = edge_counts
    n = int(off[m])
    check(ctx.pairing_batch_many(pool[0][:n], pool[1][:n], off[:m + 1]), want[:m])


def test_zero_points(ctx, pool):
    sizes = [3, 3, 3, 2, 1]
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n].copy(), pool[1][:n].copy()
    p[0] = E.zero_point(12)                    # product 0: its first pair has a zero G1
    q[5] = E.zero_point(24)                    # product 1: its last pair has a zero G2
    p[6], q[7], p[8], q[8] = E.zero_point(12), E.zero_point(24), E.zero_point(12), E.zero_point(24)  # product 2: all
    q[9] = E.zero_point(24)                    # product 3: the first of two
    want = expect(p, q, off)
    assert np.array_equal(want[2], ONE)
    assert np.array_equal(want[0], O.pairing_batch(p[1:3], q[1:3]))   # a zero pair is skipped
    check(ctx.pairing_batch_many(p, q, off), want)


def test_jacobian_and_affine_operands(ctx, pool):
    sizes = [1, 2, 3, 4] * 6
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n], pool[1][:n]
    pa, qa = O.g1_normalize(p), O.g2_normalize(q)
    assert np.array_equal(pa[0, 8:12], ONE[:4]) and np.array_equal(qa[0, 16:20], ONE[:4])
    want = expect(p, q, off)
    check(ctx.pairing_batch_many(p, q, off), want, "Jacobian")
    check(ctx.pairing_batch_many(pa, qa, off), want, "affine")      # the same points: the same Gt
    check(ctx.pairing_batch_many(pa, q, off), want, "mixed")


def test_edge_operands(ctx):
    pe, qe, _ = E.pairing_pairs()
    p64, q64 = E.one_product_terms(64)
    p2, q2 = E.one_product_terms(2)
    sizes = []
    while sum(sizes) < pe.shape[0]:
        sizes.append(min(1 + len(sizes) % 4, pe.shape[0] - sum(sizes)))
    sizes += [64, 2]
    p, q = np.concatenate([pe, p64, p2]), np.concatenate([qe, q64, q2])
    off = offsets_of(sizes)
    assert int(off[-1]) == p.shape[0] <= NPOOL
    want = expect(p, q, off)
    assert np.array_equal(want[-1], ONE) and np.array_equal(want[-2], ONE)  # e(P, Q) e(-P, Q) terms
    check(ctx.pairing_batch_many(p, q, off), want)


# ---------------------------------------------------------------- 2. paths and forms
def test_final_exponentiation_paths(own_ctx, pool):
    """The same products through the 16-lane final exponentiation (300 products: the
    default), the two-lane step machine (bn_set_fe_wide_max(0)) and, for 256 products, the
    digit-sliced blocks."""
    c = own_ctx
    c.set_products_min(0)
    sizes = [1 + (j % 7 == 0) for j in range(300)]
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    check(c.pairing_batch_many(p, q, off), want, "default")
    check(c.pairing_batch_many(p[:int(off[256])], q[:int(off[256])], off[:257]), want[:256], "digit-sliced")
    check(c.pairing_batch_many(p[:int(off[3])], q[:int(off[3])], off[:4]), want[:3], "digit-sliced, 3 products")
    c.set_fe_wide_max(0)
    check(c.pairing_batch_many(p, q, off), want, "step machine")
    check(c.pairing_batch_many(p[:int(off[3])], q[:int(off[3])], off[:4]), want[:3], "step machine, 3 products")


def test_chunking(own_ctx, pool):
    """64 terms per launch set: a product that would straddle a cut starts the next set,
    one of exactly 64 terms fills a set, empty products sit at the cuts."""
    c = own_ctx
    c.set_products_min(0)
    sizes = [30, 30, 10, 64, 0, 1, 2, 5, 56, 0, 3, 60, 4, 0, 33, 0]
    off = offsets_of(sizes)
    n = int(off[-1])
    assert 280 <= n <= 320
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    whole = c.pairing_batch_many(p, q, off)
    check(whole, want, "one launch set")
    c.set_products_chunk(64)
    check(c.pairing_batch_many(p, q, off), want, "64 terms per set")
    c.set_products_chunk(1)                    # one product per set, whatever its size
    check(c.pairing_batch_many(p, q, off), want, "one product per set")
    c.set_products_chunk(0)                    # back to the default
    check(c.pairing_batch_many(p, q, off), want, "default again")


def test_routing_of_long_and_of_few_products(own_ctx, pool):
    """Products above 64 terms take the single-product path one at a time, and so does
    every product when fewer than products_min remain; the rows are the packed path's."""
    c = own_ctx
    sizes = [2, 65, 1, 0, 4, 200, 3, 64, 0]
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    check(c.pairing_batch_many(p, q, off), want, "default products_min")
    c.set_products_min(0)
    check(c.pairing_batch_many(p, q, off), want, "packed")
    c.set_products_min(len(sizes) + 1)
    check(c.pairing_batch_many(p, q, off), want, "every product alone")
    # short products only, on either side of the crossover
    short = [j for j, s in enumerate(sizes) if s <= LANE_MAX]
    rows = np.concatenate([np.arange(off[j], off[j + 1], dtype=np.int64) for j in short])
    soff = offsets_of([sizes[j] for j in short])
    c.set_products_min(len(short))
    check(c.pairing_batch_many(p[rows], q[rows], soff), want[short], "at products_min: packed")
    c.set_products_min(len(short) + 1)
    check(c.pairing_batch_many(p[rows], q[rows], soff), want[short], "below products_min: alone")


def _dev(ctx, p, q, off, stream=None):
    import torch
    dev = torch.device("cuda", 0)
    n, m = p.shape[0], len(off) - 1
    P = torch.from_numpy(np.array(p, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev) if n else torch.zeros(12, dtype=torch.int64, device=dev)
    Q = torch.from_numpy(np.array(q, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev) if n else torch.zeros(24, dtype=torch.int64, device=dev)
    out = torch.full((max(m, 1) * 48,), 0x5a5a, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)  # the context's own stream is not ordered after torch's
    ctx.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), off, out.data_ptr(), stream)
    ctx.dev_status()  # synchronizes; raises on a sticky device outcome
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint64).reshape(-1, 48)


def test_dev_form(ctx, pool):
    sizes = [2, 0, 1, 64, 3, 70, 1]
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    check(_dev(ctx, p, q, off), want, "dev")
    # offsets are read during the call: a second call with other offsets right behind it
    import torch
    s = torch.cuda.Stream(torch.device("cuda", 0))
    check(_dev(ctx, p, q, off, s.cuda_stream), want, "dev on a caller stream")
    # n == 0: only empty products
    got = _dev(ctx, p[:0], q[:0], offsets_of([0, 0, 0]))
    check(got, np.stack([ONE] * 3), "n == 0")
    # m == 0: nothing is touched
    got = _dev(ctx, p[:0], q[:0], offsets_of([]))
    assert np.array_equal(got, np.full((1, 48), 0x5a5a, np.uint64))
    assert ctx.pairing_batch_many(p[:0], q[:0], offsets_of([])).shape == (0, 48)
    check(ctx.pairing_batch_many(p[:0], q[:0], offsets_of([0, 0])), np.stack([ONE] * 2), "host n == 0")


def test_refusals(ctx, pool):
    from substrate_bn import BnError, _native
    L, h = _native.load(), ctx.handle
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    p, q = np.array(pool[0][:6]), np.array(pool[1][:6])
    out = np.full((3, 48), 0x5a5a, np.uint64)
    vp = ctypes.c_void_p
    pp, pq, po = vp(p.ctypes.data), vp(q.ctypes.data), vp(out.ctypes.data)

    def offs(*v):
        a = np.array(v, dtype=np.uintp)
        return a, vp(a.ctypes.data)

    good, pgood = offs(0, 2, 2, 6)
    for bad in ((0, 3, 2, 6), (1, 2, 2, 6), (0, 2, 6, 5)):
        a, pa = offs(*bad)
        assert L.bn_pairing_batch_many(h, pp, pq, pa, 3, po) == INVALID, bad
        assert L.bn_pairing_batch_many_dev(h, pp, pq, pa, 3, po, None) == INVALID, bad
    assert L.bn_pairing_batch_many(h, pp, pq, None, 3, po) == INVALID
    assert L.bn_pairing_batch_many(h, None, pq, pgood, 3, po) == INVALID
    assert L.bn_pairing_batch_many(h, pp, None, pgood, 3, po) == INVALID
    assert L.bn_pairing_batch_many(h, pp, pq, pgood, 3, None) == INVALID
    assert L.bn_pairing_batch_many_dev(h, None, None, pgood, 3, None, None) == INVALID
    assert np.all(out == 0x5a5a)               # refused before any buffer is touched
    # no pairs: p and q may be NULL, out may not
    zeros, pzeros = offs(0, 0, 0, 0)
    assert L.bn_pairing_batch_many(h, None, None, pzeros, 3, po) == _native.BN_OK
    assert np.array_equal(out, np.stack([ONE] * 3))
    assert L.bn_pairing_batch_many(h, None, None, pzeros, 3, None) == INVALID
    assert L.bn_pairing_batch_many(h, None, None, None, 0, None) == _native.BN_OK   # m == 0 touches nothing
    with pytest.raises(BnError) as e:
        ctx.set_products_chunk((1 << 18) + 1)  # above kChunk
    assert e.value.code == INVALID
    ctx.set_products_chunk(1 << 18)
    ctx.set_products_chunk(0)
    # the context stays usable, at its previous settings
    check(ctx.pairing_batch_many(p, q, good), expect(p, q, good), "after the refusals")


def test_multi_device_context_shards_by_whole_products(ctx, pool):
    """Two sub-contexts on the same device: the shards are whole products, balanced by
    terms, and the rows are the single device's."""
    from substrate_bn import BnError, Context
    mctx = Context(devices=[0, 0])
    mctx.set_products_min(0)
    try:
        for sizes in ([3, 1, 0, 64, 2, 2, 5, 0], [70, 1], [0, 0, 0], [5]):
            off = offsets_of(sizes)
            n = int(off[-1])
            p, q = pool[0][:n], pool[1][:n]
            want = ctx.pairing_batch_many(p, q, off)
            check(want, expect(p, q, off), "single %s" % sizes)
            check(mctx.pairing_batch_many(p, q, off), want, "sharded %s" % sizes)
        with pytest.raises(BnError) as e:
            mctx.pairing_batch_many_dev(0, 0, [0, 0], 0)
        assert e.value.code == 1
    finally:
        mctx.close()


def _device_count():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif(_device_count() < 2, reason="needs two or more visible MI355X")
def test_sharded_over_real_devices(ctx, pool):
    from substrate_bn import Context
    nd = min(_device_count(), 4)
    mctx = Context(devices=list(range(nd)))
    mctx.set_products_min(0)
    try:
        sizes = ([0, 1, 2, 5, 0, 3, 1, 64, 1] * 4)[:33]
        off = offsets_of(sizes)
        n = int(off[-1])
        p, q = pool[0][:n], pool[1][:n]
        want = ctx.pairing_batch_many(p, q, off)
        check(want, expect(p, q, off), "single")
        check(mctx.pairing_batch_many(p, q, off), want, "sharded")
    finally:
        mctx.close()
