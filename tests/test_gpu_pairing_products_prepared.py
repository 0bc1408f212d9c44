"""Pairing products with prepared G2 terms at the C ABI (bn_pairing_batch_prepared_many and
its _dev form) against the oracle's pairing_batch over the same terms with their G2 points
written out, bit for bit on the 48 words of every row.  No tolerance is involved.

The handle holds nq = 5 points: a random Jacobian one (z != one), a normalized one, the
generator, the negation of the first, and G2::zero().  The G1 pool mixes points at z == one
with Jacobian ones.  A product is a list of terms (P index, ("f", fresh Q index) or
("i", prepared index)); `pack` turns a list of products into the call's arrays and the
written-out G2 points the oracle takes.  No launch set exceeds about 1,000 terms."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E

pytestmark = pytest.mark.gpu
NT = 16
NPOOL = 96
NQ = 5
ZQ = 4            # the handle's zero point
FRESH = 0xFFFFFFFF
ONE = np.zeros(48, np.uint64)
ONE[:4] = O.canon_to_mont_array([1]).reshape(4)
ZERO_ROW = np.zeros(48, np.uint64)
FILL = 0x5a5a5a5a5a5a5a5a
INVALID = 1
PZERO = NPOOL      # pool index of G1::zero()
QZERO = NPOOL      # fresh-pool index of G2::zero()


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    p, q, _, _ = O.random_pairs(NPOOL, seed=9307, nthreads=NT)
    p[::2] = O.g1_normalize(p[::2])                      # even entries at z == one, odd ones Jacobian
    q[::3] = O.g2_normalize(q[::3])
    assert np.array_equal(p[0, 8:12], ONE[:4]) and not np.array_equal(p[1, 8:12], ONE[:4])
    p = np.concatenate([p, E.zero_point(12).reshape(1, 12)])
    qf = np.concatenate([q, E.zero_point(24).reshape(1, 24)])
    Q = np.zeros((NQ, 24), np.uint64)
    Q[0] = q[1]
    Q[1] = O.g2_normalize(q[2:3])[0]
    Q[2] = O.g2_one()
    Q[3] = O.g2_neg(q[1:2])[0]
    Q[4] = E.zero_point(24)
    assert not np.array_equal(Q[0, 16:20], ONE[:4]) and np.array_equal(Q[1, 16:20], ONE[:4])
    for a in (p, qf, Q):
        a.setflags(write=False)
    return {"p": p, "qf": qf, "Q": Q}


@pytest.fixture(scope="module")
def prep(ctx, data):
    h = ctx.g2_prepare(data["Q"])
    assert ctx.g2_prepared_count(h) == NQ
    yield h
    ctx.g2_prepared_destroy(h)


def pack(data, products):
    """(p, compacted fresh q, qidx, offsets, written-out q) of a list of products."""
    flat = [t for terms in products for t in terms]
    off = np.zeros(len(products) + 1, np.uintp)
    off[1:] = np.cumsum([len(terms) for terms in products])
    n = len(flat)
    p = np.zeros((n, 12), np.uint64)
    qfull = np.zeros((n, 24), np.uint64)
    qidx = np.zeros(n, np.uint32)
    fresh = []
    for i, (pi, (kind, k)) in enumerate(flat):
        p[i] = data["p"][pi]
        if kind == "f":
            qidx[i] = FRESH
            qfull[i] = data["qf"][k]
            fresh.append(data["qf"][k])
        else:
            qidx[i] = k
            qfull[i] = data["Q"][k]
    q = np.stack(fresh) if fresh else np.zeros((0, 24), np.uint64)
    return p, q, qidx, off, qfull


def oracle_rows(p, qfull, off):
    def one(j):
        lo, hi = int(off[j]), int(off[j + 1])
        return O.pairing_batch(p[lo:hi], qfull[lo:hi])
    with ThreadPoolExecutor(NT) as ex:
        return np.stack(list(ex.map(one, range(off.shape[0] - 1))))


def check(got, want, what=""):
    assert got.shape == want.shape
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
    assert not bad, "%s: rows %s of %d differ" % (what, bad[:8], want.shape[0])


def host(ctx, prep, packed):
    p, q, qidx, off, _ = packed
    return ctx.pairing_batch_prepared_many(p, q, prep, qidx, off)


# ---------------------------------------------------------------- the cases
def groth16_products(m, first=0):
    """m products [fresh, 0, 1, 2]; G1::zero() at the first and the last term."""
    prods = []
    for j in range(m):
        b = first + 4 * j
        prods.append([((b + t) % NPOOL, ("f", (b // 4) % NPOOL) if t == 0 else ("i", t - 1)) for t in range(4)])
    prods[0][0] = (PZERO, prods[0][0][1])
    prods[-1][-1] = (PZERO, prods[-1][-1][1])
    return prods


def mixed_products():
    """70 products, lengths cycling 0 .. 6, the fresh term first, in the middle, last, absent
    or at every position; prepared indices run over all five points (the zero one included).
    Product 21 has every term dead (zero P, index 4, zero fresh q); the last product is
    shorter than the longest of its wave (products 64 .. 69)."""
    prods = []
    k = 0
    for j in range(70):
        L = j % 7
        v = (j // 7) % 5
        terms = []
        for t in range(L):
            if v == 4 or (v == 0 and t == 0) or (v == 1 and t == L // 2) or (v == 2 and t == L - 1):
                g2 = ("f", (k * 5 + 3) % NPOOL)
            else:
                g2 = ("i", k % NQ)
            terms.append((k % NPOOL, g2))
            k += 1
        prods.append(terms)
    prods[21] = [(PZERO, ("i", 0)), (5, ("i", ZQ)), (6, ("f", QZERO))]
    prods[69] = prods[69][:2]
    assert [len(t) for t in prods[:7]] == list(range(7)) and len(prods[69]) < max(len(t) for t in prods[64:])
    assert any(t and all(g[0] == "i" for _, g in t) for t in prods)      # an all-prepared product
    assert any(t and all(g[0] == "f" for _, g in t) for t in prods)      # an all-fresh product
    return prods


@pytest.fixture(scope="module")
def mixed(data):
    packed = pack(data, mixed_products())
    want = oracle_rows(packed[0], packed[4], packed[3])
    want.setflags(write=False)
    return packed, want


def test_groth16_shape_one_past_a_wave(ctx, data, prep):
    packed = pack(data, groth16_products(33))
    p, q, qidx, off, qfull = packed
    assert p.shape[0] == 132 and q.shape[0] == 33
    assert not p[0, 8:12].any() and not p[-1, 8:12].any()
    check(host(ctx, prep, packed), oracle_rows(p, qfull, off), "groth16 m=33")


def test_mixed_shapes_inside_a_wave(ctx, prep, mixed):
    packed, want = mixed
    assert np.array_equal(want[0], ONE) and np.array_equal(want[21], ONE)   # empty, and every term dead
    check(host(ctx, prep, packed), want, "mixed m=70")


def test_cancellation(ctx, data, prep):
    a, b = ("i", 0), ("i", 3)
    prods = [[(1, a), (1, b)], [(1, a)],
             [(1, ("f", 1)), (1, b)], [(1, ("f", 1))]]            # the fresh pool's entry 1 is Q[0]
    assert np.array_equal(data["qf"][1], data["Q"][0])
    got = host(ctx, prep, pack(data, prods))
    assert np.array_equal(got[0], ONE) and np.array_equal(got[2], ONE)
    assert not np.array_equal(got[1], ONE) and not np.array_equal(got[3], ONE)
    assert np.array_equal(got[1], got[3])
    assert np.array_equal(got[1], O.pairing_batch(data["p"][1:2], data["Q"][0:1]))


def test_a_product_of_64_terms_beside_short_ones(ctx, data, prep):
    big = [(t % NPOOL, ("f", (7 * t) % NPOOL) if t % 4 == 1 else ("i", t % 4)) for t in range(64)]
    assert sum(1 for _, g in big if g[0] == "f") == 16
    packed = pack(data, [[(3, ("i", 1)), (4, ("f", 9))], big, [(5, ("f", 2))]])
    check(host(ctx, prep, packed), oracle_rows(packed[0], packed[4], packed[3]), "64 terms")


def test_launch_set_cuts(ctx, prep, mixed):
    """Sets of at most 8 terms: they hold different fresh counts, and some none of one kind;
    wrong q or map offsets across sets would change the rows."""
    packed, want = mixed
    ctx.set_products_chunk(8)
    try:
        got = host(ctx, prep, packed)
    finally:
        ctx.set_products_chunk(0)
    check(got, want, "chunk 8")
    check(host(ctx, prep, packed), want, "default chunk again")


# ---------------------------------------------------------------- the device-pointer form
def _up(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).reshape(-1)).to(torch.device("cuda", 0))


def _out(rows):
    import torch
    return torch.full((rows * 48,), 0x5a5a, dtype=torch.int64, device=torch.device("cuda", 0))


def _rows(out):
    import torch
    torch.cuda.synchronize(torch.device("cuda", 0))
    return out.cpu().numpy().view(np.uint64).reshape(-1, 48)


def test_dev_form(ctx, data, prep):
    import torch
    prods = groth16_products(257, first=3)
    for j, terms in enumerate(prods):                       # the prepared indices vary, the zero point included
        prods[j] = [(pi, g if g[0] == "f" else ("i", (g[1] + j) % NQ)) for pi, g in terms]
    packed = pack(data, prods)
    p, q, qidx, off, qfull = packed
    assert off.shape[0] - 1 == 257
    want = ctx.pairing_batch_many(p, qfull, off)
    check(host(ctx, prep, packed), want, "host form against bn_pairing_batch_many")
    P, Qd, out = _up(p), _up(q), _out(257)
    torch.cuda.synchronize(torch.device("cuda", 0))
    ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qd.data_ptr(), prep, qidx, off, out.data_ptr())
    ctx.dev_status()                                        # BN_OK, or it raises
    check(_rows(out), want, "_dev form")
    s = torch.cuda.Stream(torch.device("cuda", 0))
    out2 = _out(257)
    torch.cuda.synchronize(torch.device("cuda", 0))
    ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qd.data_ptr(), prep, qidx, off, out2.data_ptr(), s.cuda_stream)
    ctx.dev_status(s.cuda_stream)
    check(_rows(out2), want, "_dev form on a second stream")


def test_shared_workspace_in_call_order(ctx, data, prep):
    """bn_pairing_batch_many, the new call, bn_pairing_prepared_many, the new call again, all
    enqueued on one stream with no synchronization between them."""
    import torch
    packed = pack(data, groth16_products(33))
    p, q, qidx, off, qfull = packed
    want = oracle_rows(p, qfull, off)
    idx = (np.arange(p.shape[0]) % ZQ).astype(np.uint32)
    want_pairs = O.pairing_many(p, data["Q"][idx], NT)
    P, Qf, Qd, I = _up(p), _up(qfull), _up(q), torch.from_numpy(idx.view(np.int32)).to(torch.device("cuda", 0))
    o1, o2, o3, o4 = _out(33), _out(33), _out(p.shape[0]), _out(33)
    torch.cuda.synchronize(torch.device("cuda", 0))
    ctx.pairing_batch_many_dev(P.data_ptr(), Qf.data_ptr(), off, o1.data_ptr())
    ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qd.data_ptr(), prep, qidx, off, o2.data_ptr())
    ctx.pairing_prepared_many_dev(P.data_ptr(), prep, I.data_ptr(), p.shape[0], o3.data_ptr())
    ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qd.data_ptr(), prep, qidx, off, o4.data_ptr())
    ctx.dev_status()
    check(_rows(o1), want, "bn_pairing_batch_many_dev")
    check(_rows(o2), want, "the new call")
    check(_rows(o3), want_pairs, "bn_pairing_prepared_many_dev")
    check(_rows(o4), want, "the new call again")


# ---------------------------------------------------------------- arguments
def test_refusals_touch_nothing(ctx, data, prep):
    from substrate_bn import Context, _native
    L, h = _native.load(), ctx.handle
    vp = ctypes.c_void_p
    prods = [[(1, ("f", 4)), (2, ("i", 0)), (3, ("i", 1))], [(4, ("i", 2))]]
    p, q, qidx, off, qfull = pack(data, prods)
    out = np.full((2, 48), FILL, np.uint64)
    ptr = lambda a: vp(a.ctypes.data)  # noqa: E731

    def both(hh, pp, qq, handle, ii, oo, m, po):
        rc = L.bn_pairing_batch_prepared_many(hh, pp, qq, handle, ii, oo, m, po)
        assert L.bn_pairing_batch_prepared_many_dev(hh, pp, qq, handle, ii, oo, m, po, None) == rc
        return rc

    for bad in (NQ, 0xFFFFFFFE):
        ix = qidx.copy()
        ix[2] = bad
        assert both(h, ptr(p), ptr(q), prep, ptr(ix), ptr(off), 2, ptr(out)) == INVALID
    assert both(h, ptr(p), ptr(q), prep, None, ptr(off), 2, ptr(out)) == INVALID           # NULL qidx
    assert both(h, ptr(p), None, prep, ptr(qidx), ptr(off), 2, ptr(out)) == INVALID        # NULL q, a fresh term
    assert both(h, None, ptr(q), prep, ptr(qidx), ptr(off), 2, ptr(out)) == INVALID        # NULL p, n > 0
    assert both(h, ptr(p), ptr(q), prep, ptr(qidx), ptr(off), 2, None) == INVALID          # NULL out
    assert both(h, ptr(p), ptr(q), None, ptr(qidx), ptr(off), 2, ptr(out)) == INVALID      # NULL handle
    assert both(h, ptr(p), ptr(q), prep, ptr(qidx), None, 2, ptr(out)) == INVALID          # NULL offsets
    big_p = np.tile(data["p"][1], (65, 1))
    big_i = np.zeros(65, np.uint32)
    big_off = np.array([0, 65], np.uintp)
    assert both(h, ptr(big_p), None, prep, ptr(big_i), ptr(big_off), 1, ptr(out)) == INVALID   # 65 terms
    for bad_off in ([1, 3, 4], [0, 3, 2]):                                                 # not from 0; decreasing
        o = np.array(bad_off, np.uintp)
        assert both(h, ptr(p), ptr(q), prep, ptr(qidx), ptr(o), 2, ptr(out)) == INVALID
    assert both(h, None, None, None, None, None, 0, None) == _native.BN_OK                 # m == 0 touches nothing
    other = Context(0)
    try:                                                                                   # another context's handle
        assert both(other.handle, ptr(p), ptr(q), prep, ptr(qidx), ptr(off), 2, ptr(out)) == INVALID
        gone = other.g2_prepare(data["Q"])
        other.g2_prepared_destroy(gone)                                                    # a destroyed one
        assert both(other.handle, ptr(p), ptr(q), gone, ptr(qidx), ptr(off), 2, ptr(out)) == INVALID
    finally:
        other.close()
    multi = Context(devices=[0, 0])                    # two sub-contexts on one device, as the existing tests make
    try:
        assert both(multi.handle, ptr(p), ptr(q), prep, ptr(qidx), ptr(off), 2, ptr(out)) == INVALID
        assert np.all(out == FILL)
        sub = multi.device(1)                          # a device context of it works
        hs = sub.g2_prepare(data["Q"])
        check(sub.pairing_batch_prepared_many(p, q, hs, qidx, off), oracle_rows(p, qfull, off), "device context")
        sub.g2_prepared_destroy(hs)
    finally:
        multi.close()
    assert np.all(out == FILL)
    # the handle and the context stay usable
    check(ctx.pairing_batch_prepared_many(p, q, prep, qidx, off), oracle_rows(p, qfull, off), "after the refusals")


def test_python_mirror_end_to_end(ctx, data):
    import substrate_bn as bn
    Q = [bn.G2(data["Q"][j]) for j in range(NQ)]
    P = [bn.G1(data["p"][k]) for k in range(4)]
    F = bn.G2(data["qf"][7])
    with bn.G2Prepared(Q, ctx=ctx) as prepared:
        got = bn.pairing_batch_prepared_many([[(P[0], F), (P[1], 0), (P[2], 1), (P[3], 2)], [], [(P[1], 3)]], prepared)
    want = bn.pairing_batch_many([[(P[0], F), (P[1], Q[0]), (P[2], Q[1]), (P[3], Q[2])], [], [(P[1], Q[3])]])
    assert len(got) == 3 and all(np.array_equal(g.img, w.img) for g, w in zip(got, want))
    assert np.array_equal(got[1].img, ONE)
