"""The pairing on scaled inputs (pairing.h scaled_inputs) through the kernels that run it:
k_pairing_full behind pairing_many / pairing_many_dev, and the line producers of
pairing_batch (the eight-lane and the two-lane one) -- bit for bit against the oracle,
with z = one on one or both sides, zero points and the structured pairs in the batch.
The calls whose outputs show the affine points or the exact coefficients
(g2_precompute_many, miller_loop_many, miller_loop_batch) must still give the oracle's
values on the same contexts.  tests/test_scaled_inputs_model.py checks the identity and
the formulas on the CPU.
Runs on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E

pytestmark = pytest.mark.gpu
NT = 16
NPAIR = 257


def mixed_rows(p, q, first):
    """rows first .. first + 4 become: both z = one, only P at z = one, only Q at z = one,
    zero P, zero Q (all inside the first wave's 32 pairs for first = 20)"""
    p, q = p.copy(), q.copy()
    pn, qn = O.g1_normalize(p[first:first + 3]), O.g2_normalize(q[first:first + 3])
    p[first], q[first] = pn[0], qn[0]
    p[first + 1] = pn[1]
    q[first + 2] = qn[2]
    p[first + 3] = E.zero_point(12)
    q[first + 4] = E.zero_point(24)
    return p, q


@pytest.fixture(scope="module")
def ref():
    """257 random Jacobian pairs, the same with the mixed rows in the first wave, and the
    structured pairs, with the oracle's Gt; computed once, read-only"""
    _, S = O.random_scalars(NPAIR, seed=4242, lo=1)
    p = O.g1_mul(np.tile(O.g1_one(), (NPAIR, 1)), S, NT)
    q = O.g2_mul(np.tile(O.g2_one(), (NPAIR, 1)), np.roll(S, 3, axis=0), NT)
    pm, qm = mixed_rows(p, q, 20)
    pe, qe, labels = E.pairing_pairs()
    one = O.canon_to_mont_array([1] + [0] * 11)
    d = {"p": p, "q": q, "gt": O.pairing_many(p, q, NT), "pm": pm, "qm": qm, "gtm": O.pairing_many(pm, qm, NT),
         "pe": pe, "qe": qe, "gte": O.pairing_many(pe, qe, NT), "one": one}
    assert np.array_equal(d["gtm"][23], one) and np.array_equal(d["gtm"][24], one)
    assert np.array_equal(d["gtm"][20:23], d["gt"][20:23])
    for v in d.values():
        v.setflags(write=False)
    d["labels"] = labels
    return d


@pytest.fixture(scope="module")
def ctx_tp():
    """every pairing_many batch on the throughput path (k_pairing_full)"""
    from substrate_bn import Context
    c = Context(0)
    c.set_fe_wide_max(0)
    return c


@pytest.fixture(scope="module", params=["default", "0"])
def ctx_batch(request):
    """pairing_batch's line producer: the eight-lane k_prepare_wide at its default threshold,
    the two-lane k_prepare with the threshold at 0 (read when the context is made).  The
    one-launch latency kernel is off, so every size reaches the producer."""
    from substrate_bn import Context
    with pytest.MonkeyPatch.context() as mp:
        if request.param == "0":
            mp.setenv("BN254MI_PREPARE_WIDE_MAX", "0")
        else:
            mp.delenv("BN254MI_PREPARE_WIDE_MAX", raising=False)
        c = Context(0)
    c.set_latency_max(0)
    return c


def same(got, want, what):
    bad = np.flatnonzero((got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))
    assert bad.size == 0, "%s: rows %s of %d differ" % (what, bad[:8], got.shape[0])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def rows(ref, n):
    """n = 33, 257: the batch with the mixed rows in its first wave"""
    if n >= 33:
        return ref["pm"][:n], ref["qm"][:n], ref["gtm"][:n]
    return ref["p"][:n], ref["q"][:n], ref["gt"][:n]


# ---------------------------------------------------------------- k_pairing_full
@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_pairing_many(ctx_tp, ref, n):
    p, q, want = rows(ref, n)
    same(ctx_tp.pairing_many(p, q), want, "pairing_many, n = %d" % n)


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_pairing_many_dev(ctx_tp, ref, n):
    import torch
    p, q, want = rows(ref, n)
    P, Q = _dev(p), _dev(q)
    out = torch.zeros((n, 48), dtype=torch.int64, device="cuda:0")
    ctx_tp.pairing_many_dev(P.data_ptr(), Q.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    same(out.cpu().numpy().view(np.uint64), want, "pairing_many_dev, n = %d" % n)


def test_pairing_many_structured_pairs(ctx_tp, ref):
    same(ctx_tp.pairing_many(ref["pe"], ref["qe"]), ref["gte"], "pairing_many of the structured pairs")


# ---------------------------------------------------------------- pairing_batch, both producers
def batch_rows(ref, n):
    """one zero-point term and one z = one term in every size (n = 1: the z = one term,
    and the zero-point term on its own: the product is one)"""
    if n == 1:
        return ref["pm"][20:21], ref["qm"][20:21]
    p, q = ref["pm"][:n].copy(), ref["qm"][:n].copy()
    p[0], q[0] = ref["pm"][20], ref["qm"][20]  # both z = one
    p[1], q[1] = ref["pm"][23], ref["qm"][23]  # zero P
    return p, q


@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_pairing_batch(ctx_batch, ref, n):
    p, q = batch_rows(ref, n)
    assert np.array_equal(ctx_batch.pairing_batch(p, q), O.pairing_batch(p, q, NT)), n
    if n == 1:
        assert np.array_equal(ctx_batch.pairing_batch(ref["pm"][23:24], ref["qm"][23:24]), ref["one"])
        assert np.array_equal(ctx_batch.pairing_batch(ref["pm"][24:25], ref["qm"][24:25]), ref["one"])


@pytest.mark.parametrize("n", [5, 257])
def test_pairing_batch_default_dispatch(ref, n):
    """a context as callers get it (small batches on the latency kernel)"""
    from substrate_bn import Context
    p, q = batch_rows(ref, n)
    assert np.array_equal(Context(0).pairing_batch(p, q), O.pairing_batch(p, q, NT)), n


@pytest.mark.parametrize("n", [5, 257])
def test_pairing_batch_dev(ctx_batch, ref, n):
    import torch
    p, q = batch_rows(ref, n)
    out = torch.zeros(48, dtype=torch.int64, device="cuda:0")
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    P, Q = _dev(p), _dev(q)
    ctx_batch.pairing_batch_dev(P.data_ptr(), Q.data_ptr(), n, out.data_ptr(), st.data_ptr())
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint64), O.pairing_batch(p, q, NT))


# ---------------------------------------------------------------- observable outputs stay exact
def oracle_coeffs(q):
    qa, rcs = O.g2_to_affine(q)
    assert rcs == [0] * q.shape[0]
    return np.stack([O.g2_precompute(qa[k]) for k in range(q.shape[0])])


@pytest.mark.parametrize("n", [1, 33])
def test_g2_precompute_many_stays_exact(ctx_batch, ref, n):
    q = ref["qm"][20:20 + n] if n == 1 else np.concatenate([ref["qm"][:24], ref["qm"][25:34]])  # (no zero Q)
    same(ctx_batch.g2_precompute_many(q), oracle_coeffs(q), "g2_precompute_many, n = %d" % n)


def test_miller_loop_many_stays_exact(ctx_batch, ctx_tp, ref):
    p, q = ref["p"][:33].copy(), ref["q"][:33].copy()
    p[20:23], q[20:23] = ref["pm"][20:23], ref["qm"][20:23]  # the z = one rows, no zero point
    want = np.stack([O.miller_loop_batch(q[k:k + 1], p[k:k + 1])[1] for k in range(33)])
    same(ctx_batch.miller_loop_many(p, q), want, "miller_loop_many, n = 33")
    same(ctx_tp.miller_loop_many(p, q), want, "miller_loop_many on the throughput context, n = 33")


@pytest.mark.parametrize("n", [5, 64])
def test_miller_loop_batch_stays_exact(ctx_batch, ref, n):
    p, q = ref["p"][:n].copy(), ref["q"][:n].copy()
    p[0], q[0] = ref["pm"][20], ref["qm"][20]  # both z = one
    rc, want = O.miller_loop_batch(q, p)
    assert rc == 0 and np.array_equal(ctx_batch.miller_loop_batch(q, p), want.reshape(48)), n
