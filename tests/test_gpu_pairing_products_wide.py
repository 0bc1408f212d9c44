"""The wide path of the pairing products (k_pairing_latency's Miller value per
term, k_fq12_products_wide with a 16-lane group per product, the final exponentiation) at the
C ABI against the oracle: row j is O.pairing_batch of product j's pairs, bit for bit on its 48
words.  No tolerance is involved.

Every case sets bn_set_products_wide_max itself and asserts bn_get_products_routes, the
products planned as (wide, packed, alone), beside the rows: a tree that does not take the
path fails the route assertions whatever it computes.  The prepared shapes run through both
routes, so the packed kernels behind bn_pairing_batch_prepared_many stay covered at these
sizes.  No call exceeds about 700 terms."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E

pytestmark = pytest.mark.gpu
NT = 16
NPOOL = 700
WIDE = 1 << 20     # a wide_max above every call here
FRESH = 0xFFFFFFFF
FILL = 0x5a5a
ONE = np.zeros(48, np.uint64)
ONE[:4] = O.canon_to_mont_array([1]).reshape(4)


@pytest.fixture(scope="module")
def ctx():
    """Default settings but for the threshold."""
    from substrate_bn import Context
    c = Context(0)
    c.set_products_wide_max(WIDE)
    return c


@pytest.fixture()
def own_ctx():
    """A context of the test's own, for the tests that turn knobs."""
    from substrate_bn import Context
    c = Context(0)
    c.set_products_wide_max(WIDE)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    p, q, _, _ = O.random_pairs(NPOOL, seed=8311, nthreads=NT)
    assert not np.array_equal(p[0, 8:12], ONE[:4]) and not np.array_equal(q[0, 16:20], ONE[:4])  # Jacobian
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(sizes)
    return off


def expect(p, q, off):
    """The oracle's pairing_batch of every product."""
    def one(j):
        lo, hi = int(off[j]), int(off[j + 1])
        return O.pairing_batch(p[lo:hi], q[lo:hi])
    with ThreadPoolExecutor(NT) as ex:
        rows = list(ex.map(one, range(len(off) - 1)))
    return np.stack(rows) if rows else np.zeros((0, 48), np.uint64)


def check(got, want, what=""):
    assert got.shape == want.shape
    bad = [j for j in range(want.shape[0]) if not np.array_equal(got[j], want[j])]
    assert not bad, "%s: products %s of %d differ" % (what, bad[:8], want.shape[0])


def routed(c, routes, call):
    """call() with the routes it planned asserted."""
    c.products_routes()
    got = call()
    assert c.products_routes() == routes, "routes (wide, packed, alone)"
    assert c.products_routes() == (0, 0, 0)        # the read cleared them
    return got


def fresh(c, p, q, off, routes):
    return routed(c, routes, lambda: c.pairing_batch_many(p, q, off))


# ---------------------------------------------------------------- the fresh form
@pytest.fixture(scope="module")
def edge_counts(pool):
    """33 products of one to three terms and the oracle's rows; fewer products are a prefix."""
    off = offsets_of([1 + j % 3 for j in range(33)])
    n = int(off[-1])
    return off, expect(pool[0][:n], pool[1][:n], off)


@pytest.mark.parametrize("m", [1, 2, 15, 16, 17, 33])
def test_product_counts_at_group_and_block_edges(ctx, pool, edge_counts, m):
    off, want = edge_counts
    n = int(off[m])
    routes = (0, 0, 1) if m == 1 else (m, 0, 0)    # one product keeps the single-product path
    check(fresh(ctx, pool[0][:n], pool[1][:n], off[:m + 1], routes), want[:m])


def test_sizes_mixed_inside_one_block(ctx, pool):
    sizes = [0, 1, 2, 5, 0, 3, 1, 64, 1] * 4
    off = offsets_of(sizes)
    n = int(off[-1])
    assert n <= NPOOL
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    assert all(np.array_equal(want[j], ONE) for j, s in enumerate(sizes) if s == 0)
    check(fresh(ctx, p, q, off, (len(sizes), 0, 0)), want)


def test_only_empty_products(ctx, pool):
    got = fresh(ctx, pool[0][:0], pool[1][:0], offsets_of([0] * 5), (5, 0, 0))
    check(got, np.stack([ONE] * 5))
    got = fresh(ctx, pool[0][:0], pool[1][:0], offsets_of([0] * 17), (17, 0, 0))
    check(got, np.stack([ONE] * 17))


def test_zero_points(ctx, pool):
    sizes = [3, 3, 3, 2, 1, 2]
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n].copy(), pool[1][:n].copy()
    zp, zq = E.zero_point(12), E.zero_point(24)           # (0, 1, 0)
    zp2, zq2 = pool[0][20].copy(), pool[1][20].copy()                  # z == 0 under a point's x and y
    zp2[8:12] = 0
    zq2[16:24] = 0
    p[0] = zp                                  # product 0: its first pair has a zero G1
    q[5] = zq2                                 # product 1: its last pair has a zero G2
    p[6], q[7], p[8], q[8] = zp2, zq, zp, zq2  # product 2: every pair
    q[9] = zq                                  # product 3: the first of two
    p[11] = zp2                                # product 4: its only pair
    want = expect(p, q, off)
    assert np.array_equal(want[2], ONE) and np.array_equal(want[4], ONE)
    assert np.array_equal(want[0], O.pairing_batch(p[1:3], q[1:3]))   # a zero pair is skipped
    check(fresh(ctx, p, q, off, (6, 0, 0)), want)


def test_cancelling_and_edge_products(ctx, pool):
    p2, q2 = E.one_product_terms(2)            # e(P, Q) e(-P, Q)
    p64, q64 = E.one_product_terms(64)
    p = np.concatenate([pool[0][:3], p2, p64, pool[0][3:4]])
    q = np.concatenate([pool[1][:3], q2, q64, pool[1][3:4]])
    off = offsets_of([3, 2, 64, 1])
    want = expect(p, q, off)
    assert np.array_equal(want[1], ONE) and np.array_equal(want[2], ONE)
    assert not np.array_equal(want[0], ONE)
    check(fresh(ctx, p, q, off, (4, 0, 0)), want)


def test_jacobian_and_affine_operands(ctx, pool):
    sizes = [1, 2, 3, 4] * 3
    off = offsets_of(sizes)
    n = int(off[-1])
    p, q = pool[0][:n], pool[1][:n]
    pa, qa = O.g1_normalize(p), O.g2_normalize(q)
    assert np.array_equal(pa[0, 8:12], ONE[:4]) and np.array_equal(qa[0, 16:20], ONE[:4])
    want = expect(p, q, off)
    routes = (len(sizes), 0, 0)
    check(fresh(ctx, p, q, off, routes), want, "Jacobian")
    check(fresh(ctx, pa, qa, off, routes), want, "affine")      # the same points: the same Gt
    check(fresh(ctx, pa, q, off, routes), want, "mixed")


LONG_SIZES = [2, 65, 1, 0, 4, 200, 3, 64, 0]


@pytest.fixture(scope="module")
def long_case(pool):
    off = offsets_of(LONG_SIZES)
    n = int(off[-1])
    return off, expect(pool[0][:n], pool[1][:n], off)


def test_long_products_inside_a_wide_call(ctx, pool, long_case):
    """The 65- and the 200-term product run alone; each ends the wide set in front of it."""
    off, want = long_case
    n = int(off[-1])
    check(fresh(ctx, pool[0][:n], pool[1][:n], off, (7, 0, 2)), want)


def test_final_exponentiation_forms(own_ctx, pool):
    """3 and 100 products (the digit-sliced blocks), 300 (the 16-lane groups), and 3 through
    the two-lane step machine."""
    c = own_ctx
    off = offsets_of([1 + (j % 7 == 0) for j in range(300)])
    n = int(off[-1])
    p, q = pool[0][:n], pool[1][:n]
    want = expect(p, q, off)
    for m in (3, 100, 300):
        k = int(off[m])
        check(fresh(c, p[:k], q[:k], off[:m + 1], (m, 0, 0)), want[:m], "%d products" % m)
    c.set_fe_wide_max(0)
    k = int(off[3])
    check(fresh(c, p[:k], q[:k], off[:4], (3, 0, 0)), want[:3], "step machine")


CUT_SIZES = [3, 3, 2, 0, 8, 0, 0, 5, 4, 0, 1, 7, 7]


@pytest.fixture(scope="module")
def cut_case(pool):
    off = offsets_of(CUT_SIZES)
    n = int(off[-1])
    assert n == 40
    return off, expect(pool[0][:n], pool[1][:n], off)


def test_set_cuts(own_ctx, pool, cut_case):
    """Sets of at most 8 terms, then of at most 16: a product that would straddle a cut starts
    the next set, one of exactly 8 terms fills a set, empty products sit at the cuts."""
    c = own_ctx
    off, want = cut_case
    p, q = pool[0][:40], pool[1][:40]
    m = len(CUT_SIZES)
    check(fresh(c, p, q, off, (m, 0, 0)), want, "one set")
    c.set_products_chunk(8)
    check(fresh(c, p, q, off, (m, 0, 0)), want, "8 terms per set")
    c.set_products_chunk(0)
    c.set_latency_max(16)
    check(fresh(c, p, q, off, (m, 0, 0)), want, "16 terms per set")
    c.set_latency_max(7)                       # the 8-term product is no longer eligible
    check(fresh(c, p, q, off, (m - 1, 0, 1)), want, "7 terms per set")


def test_path_off(own_ctx, pool, cut_case):
    c = own_ctx
    off, want = cut_case
    p, q = pool[0][:40], pool[1][:40]
    m = len(CUT_SIZES)                         # 13 short products: above the default products_min
    c.set_latency_max(0)
    check(fresh(c, p, q, off, (0, m, 0)), want, "latency_max 0")
    c.set_latency_max(4096)
    check(fresh(c, p, q, off, (m, 0, 0)), want, "on again")
    c.set_products_wide_max(0)
    check(fresh(c, p, q, off, (0, m, 0)), want, "wide_max 0")
    c.set_products_wide_max(39)                # one term below the call's
    check(fresh(c, p, q, off, (0, m, 0)), want, "wide_max below the call")
    c.set_products_wide_max(40)
    check(fresh(c, p, q, off, (m, 0, 0)), want, "wide_max at the call")
    c.set_products_min(0)                      # every short product packed, as documented
    check(fresh(c, p, q, off, (0, m, 0)), want, "products_min 0")
    c.set_products_min(m + 1)                  # below products_min the wide path still applies ...
    check(fresh(c, p, q, off, (m, 0, 0)), want, "below products_min")
    c.set_products_wide_max(0)                 # ... and without it every product runs alone
    check(fresh(c, p[:8], q[:8], off[:4], (0, 0, 3)), want[:3], "alone")


def _to_dev(a, width):
    import torch
    dev = torch.device("cuda", 0)
    if a.shape[0] == 0:
        return torch.zeros(width, dtype=torch.int64, device=dev)
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).reshape(-1)).to(dev)


def _out_dev(rows):
    import torch
    return torch.full((rows * 48,), FILL, dtype=torch.int64, device=torch.device("cuda", 0))


def _rows(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 48)


def test_dev_form(ctx, pool, long_case):
    import torch
    off, want = long_case
    n, m = int(off[-1]), len(LONG_SIZES)
    P, Q = _to_dev(pool[0][:n], 12), _to_dev(pool[1][:n], 24)
    for stream in (None, torch.cuda.Stream(torch.device("cuda", 0))):
        out = _out_dev(m + 2)
        torch.cuda.synchronize()               # the context's own stream is not ordered after torch's
        routed(ctx, (7, 0, 2), lambda: ctx.pairing_batch_many_dev(
            P.data_ptr(), Q.data_ptr(), off, out.data_ptr(), stream.cuda_stream if stream else None))
        ctx.dev_status(stream.cuda_stream if stream else None)  # synchronizes; raises on a sticky outcome
        torch.cuda.synchronize()
        got = _rows(out)
        check(got[:m], want, "dev")
        assert np.all(got[m:] == FILL)         # the tail of out is untouched


def test_four_calls_back_to_back_on_one_stream(own_ctx, pool, cut_case, long_case):
    """Wide, packed, wide and a single pairing_batch enqueued without a synchronize between
    them: they share the workspace, the offset words and the slots."""
    import torch
    c = own_ctx
    off, want = cut_case
    loff, lwant = long_case
    m, n = len(CUT_SIZES), int(loff[-1])
    P, Q = _to_dev(pool[0][:n], 12), _to_dev(pool[1][:n], 24)
    outs = [_out_dev(m), _out_dev(m), _out_dev(len(LONG_SIZES)), _out_dev(1)]
    s = torch.cuda.Stream(torch.device("cuda", 0))
    torch.cuda.synchronize()
    c.products_routes()
    c.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), off, outs[0].data_ptr(), s.cuda_stream)
    c.set_products_wide_max(0)
    c.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), off, outs[1].data_ptr(), s.cuda_stream)
    c.set_products_wide_max(WIDE)
    c.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), loff, outs[2].data_ptr(), s.cuda_stream)
    c.pairing_batch_dev(P.data_ptr(), Q.data_ptr(), 5, outs[3].data_ptr(), None, s.cuda_stream)
    assert c.products_routes() == (m + 7, m, 2)
    c.dev_status(s.cuda_stream)
    torch.cuda.synchronize()
    check(_rows(outs[0]), want, "wide")
    check(_rows(outs[1]), want, "packed")
    check(_rows(outs[2]), lwant, "wide with long products")
    check(_rows(outs[3]), O.pairing_batch(pool[0][:5], pool[1][:5]).reshape(1, 48), "pairing_batch")


# ---------------------------------------------------------------- the prepared form
NQ = 5
ZQ = 4             # the handle's zero point


@pytest.fixture(scope="module")
def table(pool):
    q = pool[1]
    Q = np.zeros((NQ, 24), np.uint64)
    Q[0] = q[601]                                  # Jacobian
    Q[1] = O.g2_normalize(q[602:603])[0]
    Q[2] = O.g2_one()
    Q[3] = O.g2_neg(q[601:602])[0]
    Q[4] = E.zero_point(24)
    assert not np.array_equal(Q[0, 16:20], ONE[:4]) and np.array_equal(Q[1, 16:20], ONE[:4])
    Q.setflags(write=False)
    return Q


def pack(pool, table, products):
    """products: lists of terms (pool index of P, "f" for the pool's own Q or a table index) ->
    (p, compacted fresh q, qidx, offsets, written-out q)."""
    flat = [t for terms in products for t in terms]
    off = offsets_of([len(terms) for terms in products]).astype(np.uintp)
    n = len(flat)
    p = np.zeros((n, 12), np.uint64)
    qfull = np.zeros((n, 24), np.uint64)
    qidx = np.zeros(n, np.uint32)
    for i, (pi, k) in enumerate(flat):
        p[i] = pool[0][pi] if pi >= 0 else E.zero_point(12)
        qidx[i] = FRESH if k in ("f", "z") else k
        qfull[i] = E.zero_point(24) if k == "z" else pool[1][pi] if k == "f" else table[k]
    q = qfull[qidx == FRESH]
    return p, q, qidx, off, qfull


def groth16(m):
    return [[(4 * j, "f"), (4 * j + 1, 0), (4 * j + 2, 1), (4 * j + 3, 2)] for j in range(m)]


PREPARED_SHAPES = {
    "groth16 x 1": groth16(1),
    "groth16 x 17": groth16(17),
    "groth16 x 33": groth16(33),
    "all prepared, 3 terms": [[(3 * j, j % 4), (3 * j + 1, (j + 1) % 4), (3 * j + 2, 3)] for j in range(18)],
    "all fresh": [[(5 * j + t, "f") for t in range(1 + j % 4)] for j in range(18)],
    # a zero table point, a zero fresh point, a zero P; product 2 has every term dead; an empty product;
    # e(P, Q0) e(P, -Q0) cancels
    "zeros": [[(1, ZQ), (2, "f"), (3, 0)], [(4, "z"), (5, 1)], [(6, ZQ), (7, "z"), (-1, 0)], [], [(8, 0), (8, 3)],
              [(-1, "f"), (9, 2)]],
}


@pytest.fixture(scope="module")
def prep(ctx, table):
    h = ctx.g2_prepare(table)
    yield h
    ctx.g2_prepared_destroy(h)


@pytest.mark.parametrize("shape", list(PREPARED_SHAPES))
def test_prepared_shapes_through_both_routes(ctx, pool, table, prep, shape):
    prods = PREPARED_SHAPES[shape]
    p, q, qidx, off, qfull = pack(pool, table, prods)
    m = len(prods)
    want = expect(p, qfull, off)
    if shape == "zeros":
        assert np.array_equal(want[2], ONE) and np.array_equal(want[3], ONE) and np.array_equal(want[4], ONE)
    call = lambda: ctx.pairing_batch_prepared_many(p, q, prep, qidx, off)  # noqa: E731
    try:
        wide = routed(ctx, (m, 0, 0), call)
        ctx.set_products_wide_max(0)
        packed = routed(ctx, (0, m, 0), call)
        ctx.set_products_wide_max(int(off[-1]))            # at the call's terms: wide
        wide2 = routed(ctx, (m, 0, 0), call)
        if off[-1] > 0:
            ctx.set_products_wide_max(int(off[-1]) - 1)    # one below: packed
            routed(ctx, (0, m, 0), call)
    finally:
        ctx.set_products_wide_max(WIDE)
    check(wide, want, "wide")
    check(packed, want, "packed")
    check(wide2, wide, "wide at the threshold")


def test_prepared_set_cuts(own_ctx, pool, table):
    """Sets of at most 64 terms: fresh indices restart per set and the fresh points move on."""
    c = own_ctx
    h = c.g2_prepare(table)
    prods = groth16(33) + [[(140 + t, "f" if t % 3 == 0 else t % 4) for t in range(64)]]
    p, q, qidx, off, qfull = pack(pool, table, prods)
    want = expect(p, qfull, off)
    call = lambda: c.pairing_batch_prepared_many(p, q, h, qidx, off)  # noqa: E731
    check(routed(c, (34, 0, 0), call), want, "one set")
    c.set_products_chunk(64)
    check(routed(c, (34, 0, 0), call), want, "64 terms per set")
    c.set_products_chunk(63)                   # a 64-term product would not fit a set: packed
    check(routed(c, (0, 34, 0), call), want, "63 terms per set")
    c.set_products_chunk(0)
    c.set_latency_max(64)
    check(routed(c, (34, 0, 0), call), want, "latency_max 64")
    c.set_latency_max(0)
    check(routed(c, (0, 34, 0), call), want, "latency_max 0")


def test_prepared_dev_form(ctx, pool, table, prep):
    import torch
    prods = groth16(17) + PREPARED_SHAPES["zeros"]
    p, q, qidx, off, qfull = pack(pool, table, prods)
    m = len(prods)
    want = expect(p, qfull, off)
    P, Q = _to_dev(p, 12), _to_dev(q, 24)
    for stream in (None, torch.cuda.Stream(torch.device("cuda", 0))):
        out = _out_dev(m + 1)
        torch.cuda.synchronize()
        routed(ctx, (m, 0, 0), lambda: ctx.pairing_batch_prepared_many_dev(
            P.data_ptr(), Q.data_ptr(), prep, qidx, off, out.data_ptr(), stream.cuda_stream if stream else None))
        ctx.dev_status(stream.cuda_stream if stream else None)
        torch.cuda.synchronize()
        got = _rows(out)
        check(got[:m], want, "prepared dev")
        assert np.all(got[m:] == FILL)


def test_handle_lifecycle(own_ctx, pool, table):
    """Destroy after a wide call; a second handle with other points; a handle made by
    bn_g2_prepare_dev; the context frees the one still alive."""
    import torch
    c = own_ctx
    prods = groth16(5)
    p, q, qidx, off, qfull = pack(pool, table, prods)
    want = expect(p, qfull, off)
    h1 = c.g2_prepare(table)
    check(routed(c, (5, 0, 0), lambda: c.pairing_batch_prepared_many(p, q, h1, qidx, off)), want, "first handle")
    other = np.array(table[[2, 0, 1, 3, 4]])
    h2 = c.g2_prepare(other)
    c.g2_prepared_destroy(h1)
    p2, q2, qidx2, off2, qfull2 = pack(pool, other, prods)
    want2 = expect(p2, qfull2, off2)
    assert not np.array_equal(want2, want)
    check(routed(c, (5, 0, 0), lambda: c.pairing_batch_prepared_many(p2, q2, h2, qidx2, off2)), want2, "second handle")
    T = _to_dev(table, 24)
    torch.cuda.synchronize()
    h3 = c.g2_prepare_dev(T.data_ptr(), NQ)
    assert c.g2_prepared_count(h3) == NQ
    check(routed(c, (5, 0, 0), lambda: c.pairing_batch_prepared_many(p, q, h3, qidx, off)), want, "device-made handle")
    c.set_products_wide_max(0)
    check(routed(c, (0, 5, 0), lambda: c.pairing_batch_prepared_many(p, q, h3, qidx, off)), want, "its table")
    c.g2_prepared_destroy(h2)


# ---------------------------------------------------------------- multi-device
def test_multi_device_context(ctx, pool):
    """Two sub-contexts on the same device: the setter reaches both, each shard of whole
    products takes the path, the counts are summed, the rows are the single device's."""
    from substrate_bn import Context
    mctx = Context(devices=[0, 0])
    try:
        off = offsets_of([3] * 12)
        n = int(off[-1])
        p, q = pool[0][:n], pool[1][:n]
        want = expect(p, q, off)
        mctx.set_products_wide_max(0)
        check(fresh(mctx, p, q, off, (0, 0, 12)), want, "off: each shard below products_min")
        mctx.set_products_wide_max(WIDE)
        check(fresh(mctx, p, q, off, (12, 0, 0)), want, "sharded")
        check(fresh(ctx, p, q, off, (12, 0, 0)), want, "single")
    finally:
        mctx.close()
