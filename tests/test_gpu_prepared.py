"""Pairings against prepared G2 points at the C ABI (bn_g2_prepare, bn_pairing_prepared_many,
bn_pairing_prepared_many_dev, bn_miller_loop_prepared_many) against the oracle, bit for bit
on the 48 words of every row.  No tolerance is involved.

The handle holds nq = 5 points: a random Jacobian one (z != one), a normalized one, the
generator, the negation of the first, and G2::zero().  P is mixed: the first 32 at z == one
(a whole wave: the Miller form's wave-uniform shortcut), the rest Jacobian at z != one, and
G1::zero() at positions 0, 33 and n - 1 where they exist.  The oracle's rows are computed
once, for every (P, live Q), and shared.

Table contents: the Miller value of a lone lane pair is the product of all 87 lines, so a
single line cannot be read back from it; the table is instead tied to bn_g2_precompute_many's
rows through the whole value -- the oracle's G2Precomp::miller_loop over the EXPORTED
coefficients must give the prepared Miller value, at points whose x and y differ."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E

pytestmark = pytest.mark.gpu
NT = 16
NP = 257
NQ = 5
ZQ = 4            # the handle's zero point
ONE = np.zeros(48, np.uint64)
ONE[:4] = O.canon_to_mont_array([1]).reshape(4)
ZERO_ROW = np.zeros(48, np.uint64)
FILL = 0x5a5a5a5a5a5a5a5a
INVALID = 1


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    """The five Q, 257 P (no zeros yet) and the oracle's pairing and Miller value of every
    (P[i], Q[j]), j < 4."""
    p, q, _, _ = O.random_pairs(NP, seed=9201, nthreads=NT)
    p[:32] = O.g1_normalize(p[:32])
    assert np.array_equal(p[31, 8:12], ONE[:4]) and not np.array_equal(p[32, 8:12], ONE[:4])
    Q = np.zeros((NQ, 24), np.uint64)
    Q[0] = q[0]
    Q[1] = O.g2_normalize(q[1:2])[0]
    Q[2] = O.g2_one()
    Q[3] = O.g2_neg(q[0:1])[0]
    Q[4] = E.zero_point(24)
    assert not np.array_equal(Q[0, 16:20], ONE[:4]) and np.array_equal(Q[1, 16:20], ONE[:4])
    gt = np.stack([O.pairing_many(p, np.tile(Q[j], (NP, 1)), NT) for j in range(ZQ)])
    pa, rp = O.g1_to_affine(p)
    qa, rq = O.g2_to_affine(Q[:ZQ])
    assert not any(rp) and not any(rq)
    coeffs = [O.g2_precompute(qa[j]) for j in range(ZQ)]
    with ThreadPoolExecutor(NT) as ex:
        ml = np.stack([np.stack(list(ex.map(lambda i, c=coeffs[j]: O.miller_loop(c, pa[i, :4], pa[i, 4:]), range(NP))))
                       for j in range(ZQ)])
    for a in (p, Q, gt, ml, qa):
        a.setflags(write=False)
    return {"p": p, "Q": Q, "gt": gt, "ml": ml, "qa": qa}


@pytest.fixture(scope="module")
def prep(ctx, data):
    h = ctx.g2_prepare(data["Q"])
    assert ctx.g2_prepared_count(h) == NQ
    yield h
    ctx.g2_prepared_destroy(h)


def points(data, n, zeros=True):
    p = data["p"][:n].copy()
    if zeros:
        for k in (0, 33, n - 1):
            if k < n:
                p[k] = E.zero_point(12)
    return p


IDX = {
    "null": lambda n: None,
    "all3": lambda n: np.full(n, 3, np.uint32),
    "mixed": lambda n: (np.arange(n) % NQ).astype(np.uint32),                # differs inside a wave, zero Q included
    "per_wave": lambda n: ((np.arange(n) // 32) % NQ).astype(np.uint32),     # constant per wave of 32 pairs
}


def expect(table, p, idx):
    n = p.shape[0]
    ix = np.zeros(n, np.uint32) if idx is None else idx
    out = np.zeros((n, 48), np.uint64)
    for i in range(n):
        dead = not p[i, 8:12].any() or ix[i] == ZQ
        out[i] = ONE if dead else table[ix[i], i]
    return out


def check(got, want, what=""):
    assert got.shape == want.shape
    bad = [i for i in range(want.shape[0]) if not np.array_equal(got[i], want[i])]
    assert not bad, "%s: rows %s of %d differ" % (what, bad[:8], want.shape[0])


# ---------------------------------------------------------------- table contents
def test_table_holds_the_exported_coefficients(ctx, data):
    exported = ctx.g2_precompute_many(data["Q"][:ZQ])                      # (4, 87, 24)
    probes = np.stack([O.g1_one(), data["p"][1], data["p"][40]])           # z == one twice, then Jacobian
    pa, _ = O.g1_to_affine(probes)
    for j in range(ZQ):
        h = ctx.g2_prepare(data["Q"][j:j + 1])
        try:
            assert ctx.g2_prepared_count(h) == 1
            got = ctx.miller_loop_prepared_many(probes, h)
            check(got, ctx.miller_loop_many(probes, np.tile(data["Q"][j], (3, 1))), "miller_loop_many, Q %d" % j)
            want = np.stack([O.miller_loop(exported[j], pa[k, :4], pa[k, 4:]) for k in range(3)])
            check(got, want, "the oracle's loop over the exported row, Q %d" % j)
            assert np.array_equal(exported[j], O.g2_precompute(data["qa"][j]))
        finally:
            ctx.g2_prepared_destroy(h)


# ---------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("case", sorted(IDX))
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 257])
def test_pairing_parity(ctx, data, prep, n, case):
    p, idx = points(data, n), IDX[case](n)
    want = expect(data["gt"], p, idx)
    assert np.array_equal(want[0], ONE) and np.array_equal(want[n - 1], ONE)
    check(ctx.pairing_prepared_many(p, prep, idx), want, "n=%d %s" % (n, case))


@pytest.mark.parametrize("case", sorted(IDX))
@pytest.mark.parametrize("n", [1, 2, 31])
def test_pairing_parity_of_live_rows_at_the_smallest_sizes(ctx, data, prep, n, case):
    """n = 1 and 2 above hold only zero P: the same sizes, and 31, with every P live."""
    p, idx = points(data, n, zeros=False), IDX[case](n)
    check(ctx.pairing_prepared_many(p, prep, idx), expect(data["gt"], p, idx), "n=%d %s" % (n, case))


@pytest.mark.parametrize("case", sorted(IDX))
@pytest.mark.parametrize("n", [33, 257])
def test_miller_parity(ctx, data, prep, n, case):
    p, idx = points(data, n), IDX[case](n)
    want = expect(data["ml"], p, idx)
    check(ctx.miller_loop_prepared_many(p, prep, idx), want, "n=%d %s" % (n, case))
    if n == 33:   # a lone wave of live Jacobian P next to a wave at z == one: no shortcut in the second
        live = points(data, n, zeros=False)
        check(ctx.miller_loop_prepared_many(live, prep, idx), expect(data["ml"], live, idx), "live n=33 %s" % case)


def test_python_mirror_end_to_end(ctx, data):
    import substrate_bn as bn
    with bn.G2Prepared([bn.G2(data["Q"][j]) for j in range(NQ)], ctx=ctx) as prepared:
        assert len(prepared) == NQ
        ps = [bn.G1(data["p"][i]) for i in (1, 40, 41)]
        got = bn.pairing_prepared_many(ps, prepared, [2, 0, ZQ])
        assert got == [bn.Gt(data["gt"][2, 1]), bn.Gt(data["gt"][0, 40]), bn.Gt.one()]
        ml = bn.miller_loop_prepared_many(ps[:2], prepared)
        assert ml == [bn.Gt(data["ml"][0, 1]), bn.Gt(data["ml"][0, 40])]
    assert prepared.closed


# ---------------------------------------------------------------- past one launch set
def test_engine_self_agreement_past_a_chunk(ctx, data, prep):
    n = (1 << 18) + 33
    p64 = points(data, 64)                       # zeros at 0, 33, 63
    p = np.ascontiguousarray(np.tile(p64, ((n + 63) // 64, 1))[:n])
    i = np.arange(n)
    idx = ((i * 7 + i // 64) % 4).astype(np.uint32)
    idx[n - 5] = ZQ
    got = ctx.pairing_prepared_many(p, prep, idx)
    want = ctx.pairing_many(p, data["Q"][idx])
    assert np.array_equal(got, want)
    assert np.array_equal(got[n - 5], ONE) and np.array_equal(got[64], ONE) and not np.array_equal(got[n - 1], ONE)
    # spot rows on both sides of the cut against the oracle's table
    for r in (1, 65, (1 << 18) - 2, (1 << 18) + 1, n - 1):
        assert p[r, 8:12].any()
        assert np.array_equal(got[r], data["gt"][idx[r], r % 64]), r


# ---------------------------------------------------------------- the device-pointer form
def _up(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64).reshape(-1)).to(torch.device("cuda", 0))


def _dev(ctx, p, handle, idx, stream=None, status=True):
    import torch
    dev = torch.device("cuda", 0)
    n = p.shape[0]
    P = _up(p)
    I = None if idx is None else torch.from_numpy(idx.astype(np.uint32).view(np.int32)).to(dev)
    out = torch.full((n * 48,), 0x5a5a, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)   # the context's own stream is not ordered after torch's
    ctx.pairing_prepared_many_dev(P.data_ptr(), handle, None if I is None else I.data_ptr(), n, out.data_ptr(), stream)
    if status:
        ctx.dev_status()          # synchronizes; raises on a sticky device outcome
    return out, (P, I)


def _rows(out):
    import torch
    torch.cuda.synchronize(torch.device("cuda", 0))
    return out.cpu().numpy().view(np.uint64).reshape(-1, 48)


def test_dev_form_on_two_streams(ctx, data, prep):
    import torch
    p = points(data, NP)
    for case in ("mixed", "null"):
        idx = IDX[case](NP)
        host = ctx.pairing_prepared_many(p, prep, idx)
        check(host, expect(data["gt"], p, idx), "host %s" % case)
        out, _keep = _dev(ctx, p, prep, idx)
        check(_rows(out), host, "context stream %s" % case)
        s = torch.cuda.Stream(torch.device("cuda", 0))
        out, _keep = _dev(ctx, p, prep, idx, s.cuda_stream)
        check(_rows(out), host, "second stream %s" % case)


def test_dev_form_bad_indices(ctx, data, prep):
    from substrate_bn import BnError
    p = points(data, NP)
    idx = IDX["mixed"](NP)
    want = expect(data["gt"], p, idx)
    idx[5], idx[100] = NQ, 0xFFFFFFFF
    out, _keep = _dev(ctx, p, prep, idx, status=False)
    with pytest.raises(BnError) as e:
        ctx.dev_status()
    assert e.value.code == INVALID
    ctx.dev_status()                                # cleared: BN_OK now
    got = _rows(out)
    assert np.array_equal(got[5], ZERO_ROW) and np.array_equal(got[100], ZERO_ROW)
    keep = [i for i in range(NP) if i not in (5, 100)]
    check(got[keep], want[keep], "the other rows")


def test_prepare_dev_builds_the_same_table(ctx, data, prep):
    import torch
    Qd = _up(data["Q"])
    torch.cuda.synchronize(torch.device("cuda", 0))
    h = ctx.g2_prepare_dev(Qd.data_ptr(), NQ)
    try:
        assert ctx.g2_prepared_count(h) == NQ
        p, idx = points(data, 33), IDX["mixed"](33)
        check(ctx.miller_loop_prepared_many(p, h, idx), expect(data["ml"], p, idx), "miller")
        check(ctx.pairing_prepared_many(p, h, idx), expect(data["gt"], p, idx), "pairing")
    finally:
        ctx.g2_prepared_destroy(h)


# ---------------------------------------------------------------- arguments
def test_refusals_touch_nothing(ctx, data, prep):
    from substrate_bn import Context, _native
    L, h = _native.load(), ctx.handle
    vp = ctypes.c_void_p
    n = 6
    p = points(data, n, zeros=False)
    out = np.full((n, 48), FILL, np.uint64)
    pp, po = vp(p.ctypes.data), vp(out.ctypes.data)
    good = np.array([0, 1, 2, 3, 4, 0], np.uint32)
    for bad_at, bad in ((0, NQ), (5, NQ), (3, 0xFFFFFFFF)):
        idx = good.copy()
        idx[bad_at] = bad
        pi = vp(idx.ctypes.data)
        assert L.bn_pairing_prepared_many(h, pp, prep, pi, n, po) == INVALID
        assert L.bn_miller_loop_prepared_many(h, pp, prep, pi, n, po) == INVALID
    pi = vp(good.ctypes.data)
    for fn in (L.bn_pairing_prepared_many, L.bn_miller_loop_prepared_many):
        assert fn(h, None, prep, pi, n, po) == INVALID
        assert fn(h, pp, prep, pi, n, None) == INVALID
        assert fn(h, pp, None, pi, n, po) == INVALID
        assert fn(h, None, None, None, 0, None) == _native.BN_OK            # n == 0 touches nothing
    assert L.bn_pairing_prepared_many_dev(h, None, prep, None, n, po, None) == INVALID
    assert L.bn_pairing_prepared_many_dev(h, pp, None, None, n, po, None) == INVALID
    assert L.bn_pairing_prepared_many_dev(h, pp, prep, None, n, None, None) == INVALID
    assert L.bn_pairing_prepared_many_dev(h, None, None, None, 0, None, None) == _native.BN_OK
    # bn_g2_prepare: nq = 0 and 2^16 + 1, NULL q and out -- and no handle comes back
    q = np.array(data["Q"])
    for fn, extra in ((L.bn_g2_prepare, ()), (L.bn_g2_prepare_dev, (None,))):
        for args in ((vp(q.ctypes.data), 0), (vp(q.ctypes.data), (1 << 16) + 1), (None, NQ)):
            hh = vp(0x1234)
            assert fn(h, args[0], args[1], ctypes.byref(hh), *extra) == INVALID
            assert not hh.value
        assert fn(h, vp(q.ctypes.data), NQ, None, *extra) == INVALID
    assert L.bn_g2_prepared_count(None) == 0
    # a handle used with another context, and destroyed through it
    other = Context(0)
    try:
        assert L.bn_pairing_prepared_many(other.handle, pp, prep, pi, n, po) == INVALID
        assert L.bn_miller_loop_prepared_many(other.handle, pp, prep, pi, n, po) == INVALID
        assert L.bn_pairing_prepared_many_dev(other.handle, pp, prep, None, n, po, None) == INVALID
        assert L.bn_g2_prepared_destroy(other.handle, prep) == INVALID
    finally:
        other.close()
    assert L.bn_g2_prepared_destroy(h, None) == INVALID
    assert np.all(out == FILL)
    # the handle and the context stay usable
    check(ctx.pairing_prepared_many(p, prep, good), expect(data["gt"], p, good), "after the refusals")


def _multi_refuses(devices, data, prep):
    from substrate_bn import Context, _native
    L = _native.load()
    vp = ctypes.c_void_p
    p = points(data, 4, zeros=False)
    out = np.full((4, 48), FILL, np.uint64)
    q = np.array(data["Q"])
    m = Context(devices=devices)
    try:
        hh = vp(0x1234)
        assert L.bn_g2_prepare(m.handle, vp(q.ctypes.data), NQ, ctypes.byref(hh)) == INVALID and not hh.value
        assert L.bn_g2_prepare_dev(m.handle, vp(q.ctypes.data), NQ, ctypes.byref(hh), None) == INVALID
        for fn in (L.bn_pairing_prepared_many, L.bn_miller_loop_prepared_many):
            assert fn(m.handle, vp(p.ctypes.data), prep, None, 4, vp(out.ctypes.data)) == INVALID
        assert L.bn_pairing_prepared_many_dev(m.handle, vp(p.ctypes.data), prep, None, 4, vp(out.ctypes.data), None) == INVALID
        assert np.all(out == FILL)
        # a device context of the multi-device one works
        sub = m.device(len(devices) - 1)
        h = sub.g2_prepare(q)
        check(sub.pairing_prepared_many(p, h, None), expect(data["gt"], p, None), "device context")
        sub.g2_prepared_destroy(h)
    finally:
        m.close()


def test_multi_device_context_is_refused(data, prep):
    """Two sub-contexts on the same device: refused as any multi-device context is."""
    _multi_refuses([0, 0], data, prep)


def _device_count():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif(_device_count() < 2, reason="needs two or more visible MI355X")
def test_multi_device_context_over_real_devices_is_refused(data, prep):
    _multi_refuses([0, 1], data, prep)


# ---------------------------------------------------------------- lifetime
def test_two_handles_alive_at_once(ctx, data):
    a = ctx.g2_prepare(data["Q"][0:2])
    b = ctx.g2_prepare(data["Q"][2:4])
    p = points(data, 33, zeros=False)
    idx = (np.arange(33) % 2).astype(np.uint32)
    want_a = expect(data["gt"], p, idx)
    want_b = expect(data["gt"], p, idx + 2)
    for _ in range(2):
        check(ctx.pairing_prepared_many(p, a, idx), want_a, "a")
        check(ctx.pairing_prepared_many(p, b, idx), want_b, "b")
    ctx.g2_prepared_destroy(a)
    check(ctx.pairing_prepared_many(p, b, idx), want_b, "b after a is gone")
    from substrate_bn import BnError
    with pytest.raises(BnError) as e:
        ctx.pairing_prepared_many(p, a, idx)        # a destroyed handle is not a live handle
    assert e.value.code == INVALID
    ctx.g2_prepared_destroy(b)


def test_destroying_the_context_frees_a_live_handle(data):
    from substrate_bn import _native
    L = _native.load()
    vp = ctypes.c_void_p
    c, h = vp(), vp()
    assert L.bn_ctx_create(0, ctypes.byref(c)) == 0
    q = np.array(data["Q"])
    p = points(data, 3, zeros=False)
    out = np.zeros((3, 48), np.uint64)
    assert L.bn_g2_prepare(c, vp(q.ctypes.data), NQ, ctypes.byref(h)) == 0 and h.value
    assert L.bn_pairing_prepared_many(c, vp(p.ctypes.data), h, None, 3, vp(out.ctypes.data)) == 0
    check(out, expect(data["gt"], p, None), "before the context goes")
    assert L.bn_ctx_destroy(c) == 0


# ---------------------------------------------------------------- the shared workspace afterwards
def test_pairing_many_after_the_new_calls(ctx, data, prep):
    """A _dev call leaves its sticky bit unread; the next host call starts from a clear word
    and the workspace the new kernel shares is intact."""
    p = points(data, 33)
    idx = IDX["mixed"](33)
    idx[7] = NQ
    out, _keep = _dev(ctx, p, prep, idx, status=False)
    q = np.array(data["Q"][[0] * 33])
    got = ctx.pairing_many(p, q)
    check(got, expect(data["gt"], p, None), "bn_pairing_many")
    assert np.array_equal(_rows(out)[7], ZERO_ROW)
    ctx.dev_status()                                # the host call cleared the word
