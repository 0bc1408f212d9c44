"""The Miller loop's line steps on merged and addend-taking column chains (curve.h
doubling_step / mixed_addition_step with BN_LINE_CHAIN, fq2_split.h "line-step chains")
through the kernels of kernels_pairing.hip that run them: the two-lane k_prepare (all
87 x 3 line coefficients, so every step's three outputs and, through the next step, its
R), k_miller behind miller_loop_many, and the throughput path's k_pairing_full behind
pairing_many and pairing_batch -- bit for bit against the oracle.  Every rewritten
quantity keeps its residue mod p, so nothing else may change.
tests/test_line_chain_model.py checks the chains' text and the two-lane formulas digit
by digit on the CPU.
Runs on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E

pytestmark = pytest.mark.gpu
NT = 16
NPAIR = 257


@pytest.fixture(scope="module")
def ctx_prepare():
    """g2_precompute_many on the two-lane k_prepare at every size: the eight-lane
    prepare kernel's threshold is read from the environment when the context is made"""
    from substrate_bn import Context
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BN254MI_PREPARE_WIDE_MAX", "0")
        c = Context(0)
    return c


@pytest.fixture(scope="module")
def ctx_tp():
    """every pairing_many batch on the throughput path (k_pairing_full)"""
    from substrate_bn import Context
    c = Context(0)
    c.set_fe_wide_max(0)
    return c


@pytest.fixture(scope="module")
def ref():
    """257 random pairs in Jacobian form and the structured pairs of edge_vectors, with
    the oracle's Miller values and Gt; computed once, read-only"""
    _, S = O.random_scalars(NPAIR, seed=9191, lo=1)
    p = O.g1_mul(np.tile(O.g1_one(), (NPAIR, 1)), S, NT)
    q = O.g2_mul(np.tile(O.g2_one(), (NPAIR, 1)), np.roll(S, 5, axis=0), NT)
    pe, qe, labels = E.pairing_pairs()
    d = {"p": p, "q": q, "gt": O.pairing_many(p, q, NT), "pe": pe, "qe": qe, "gte": O.pairing_many(pe, qe, NT)}
    for v in d.values():
        v.setflags(write=False)
    d["labels"] = labels
    return d


def oracle_coeffs(q):
    qa, rcs = O.g2_to_affine(q)
    assert rcs == [0] * q.shape[0]
    return np.stack([O.g2_precompute(qa[k]) for k in range(q.shape[0])])


def same(got, want, what):
    bad = np.flatnonzero((got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)).any(axis=1))
    assert bad.size == 0, "%s: rows %s of %d differ" % (what, bad[:8], got.shape[0])


@pytest.mark.parametrize("n", [1, 2, 33, 257])
def test_prepare_two_lane_random(ctx_prepare, ref, n):
    """random Jacobian Q, the generator (z == one) in the last row of the larger sizes"""
    q = ref["q"][:n].copy()
    if n > 2:
        q[n - 1] = np.array(O.g2_one()).reshape(24)
    got = ctx_prepare.g2_precompute_many(q)
    assert got.shape == (n, 87, 24)
    same(got, oracle_coeffs(q), "g2_precompute_many, n = %d" % n)


def test_prepare_two_lane_generator(ctx_prepare):
    q = np.array(O.g2_one()).reshape(1, 24)
    same(ctx_prepare.g2_precompute_many(q), oracle_coeffs(q), "g2_precompute_many of the generator")


def test_prepare_two_lane_edges(ctx_prepare):
    """k * G2 and (r - k) * G2 at z == one, and the same points rescaled to every structured z"""
    qa, _ = E.g2_affine_jac()
    qr, _, _ = E.g2_rescaled()
    q = np.concatenate([qa, qr])
    same(ctx_prepare.g2_precompute_many(q), oracle_coeffs(q), "g2_precompute_many of the structured points")


@pytest.mark.parametrize("n", [1, 33, 257])
def test_miller_loop_many(ctx_tp, ref, n):
    p, q = ref["p"][:n], ref["q"][:n]
    want = np.stack([O.miller_loop_batch(q[k:k + 1], p[k:k + 1])[1] for k in range(n)])
    same(ctx_tp.miller_loop_many(p, q), want, "miller_loop_many, n = %d" % n)


@pytest.mark.parametrize("n", [1, 33, 257])
def test_pairing_many_throughput(ctx_tp, ref, n):
    same(ctx_tp.pairing_many(ref["p"][:n], ref["q"][:n]), ref["gt"][:n], "pairing_many, n = %d" % n)


def test_structured_pairs(ctx_tp, ref):
    pe, qe = ref["pe"], ref["qe"]
    same(ctx_tp.pairing_many(pe, qe), ref["gte"], "pairing_many of the structured pairs")
    want = np.stack([O.miller_loop_batch(qe[k:k + 1], pe[k:k + 1])[1] for k in range(pe.shape[0])])
    same(ctx_tp.miller_loop_many(pe, qe), want, "miller_loop_many of the structured pairs")


@pytest.mark.parametrize("n", [5, 64])
def test_pairing_batch(ctx_tp, ref, n):
    p, q = ref["p"][:n], ref["q"][:n]
    assert np.array_equal(ctx_tp.pairing_batch(p, q), O.pairing_batch(p, q, NT))
