"""One product of bn_pairing_batch_prepared_many on the host: a fresh term's lines as the
producers store them, a prepared term's as k_prepared_expand writes them (pairing.h
prepared_line_scaled over the table's unscaled lines, Gt form: ell_0 Z^3, ell_vw Y, ell_vv X Z
of the Jacobian P), looked up through the per-term map and multiplied in by
miller_product_scaled (tests/native/products_prepared_emul.cpp, the one-lane layout, with the
fold-bound checks of BN_HOST_CHECKS, which abort the process).

The product has 4 terms, the Groth16 shape: one fresh affine pair and three prepared points
whose table rows are the oracle's g2_precompute.
  - every P at z == one: the Miller value is the oracle's miller_loop_batch, bit for bit;
  - the prepared terms' P Jacobian at z != one: the Miller value differs from that (by a power
    of each Z) and its oracle final_exponentiation is the oracle's pairing_batch;
  - a dead prepared term and the padding past the product's own count (iterate > K) leave the
    value unchanged;
  - the loop fetches 87 lines per term it iterates over.
The kernels around this are checked end to end by tests/test_gpu_pairing_products_prepared.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.native import productspreparedemul as E

K = 4
LINES = 87


@pytest.fixture(scope="module")
def data():
    p, q, _, _ = O.random_pairs(K, seed=8207, nthreads=4)
    pa, rp = O.g1_to_affine(p)
    qa, rq = O.g2_to_affine(q)
    assert not any(rp) and not any(rq)
    one = O.canon_to_mont_array([1]).reshape(4)
    assert not any(np.array_equal(p[k, 8:12], one) for k in range(K))   # Jacobian, z != one
    pn = O.g1_normalize(p)                                               # the same points at z == one
    table = np.stack([O.g2_precompute(qa[j]) for j in (1, 2, 3)])        # the prepared points: Q[1 .. 3]
    rc, ml = O.miller_loop_batch(q, p)
    assert rc == 0
    gt = O.pairing_batch(p, q)
    for a in (p, q, pa, qa, pn, table, ml, gt):
        a.setflags(write=False)
    return {"p": p, "q": q, "pa": pa, "qa": qa, "pn": pn, "table": table, "ml": ml, "gt": gt}


def _terms(d, pj, fresh_at=0):
    """The product's terms with the fresh pair (P[0], Q[0]) at position fresh_at and the
    prepared terms (pj[k], table row k - 1) around it in order."""
    prepared = [("prepared", pj[k], k - 1) for k in (1, 2, 3)]
    return prepared[:fresh_at] + [("fresh", d["pa"][0], d["qa"][0])] + prepared[fresh_at:]


@pytest.mark.parametrize("fresh_at", [0, 2, 3])
def test_at_z_one_the_value_is_the_oracles_miller_loop_batch(data, fresh_at):
    got, fetched = E.miller_product(_terms(data, data["pn"], fresh_at), data["table"])
    assert fetched == K * LINES
    order = [1, 2, 3]
    order.insert(fresh_at, 0)
    rc, want = O.miller_loop_batch(data["q"][order], data["p"][order])
    assert rc == 0
    assert np.array_equal(got, want)
    if fresh_at == 0:
        assert np.array_equal(got, data["ml"])


def test_jacobian_p_changes_the_miller_value_but_not_the_pairing(data):
    got, fetched = E.miller_product(_terms(data, data["p"]), data["table"])
    assert fetched == K * LINES
    assert not np.array_equal(got, data["ml"])        # off by Z^3 per line of each prepared term
    out, _ = O.final_exponentiation(got)
    assert np.array_equal(out[0], data["gt"])


@pytest.mark.parametrize("which", ["p", "pn"])
def test_a_dead_prepared_term_takes_the_line_one(data, which):
    terms = _terms(data, data[which])
    got, _ = E.miller_product(terms, data["table"], dead=[0, 0, 1, 0])
    live = [0, 1, 3]
    base, _ = E.miller_product([terms[t] for t in live], data["table"])
    assert np.array_equal(got, base)                    # the value itself is unchanged by the line one
    out, _ = O.final_exponentiation(got)
    assert np.array_equal(out[0], O.pairing_batch(data["p"][live], data["q"][live]))
    if which == "pn":
        rc, ml = O.miller_loop_batch(data["q"][live], data["p"][live])
        assert rc == 0 and np.array_equal(got, ml)


def test_padding_past_the_products_own_count_changes_nothing(data):
    terms = _terms(data, data["p"])
    base, f0 = E.miller_product(terms, data["table"])
    padded, f1 = E.miller_product(terms, data["table"], iterate=K + 3)
    assert f0 == K * LINES and f1 == (K + 3) * LINES    # the padded loop did run the extra terms
    assert np.array_equal(padded, base)


def test_every_term_dead_gives_one(data):
    got, fetched = E.miller_product(_terms(data, data["p"]), data["table"], dead=[1, 1, 1, 1], iterate=K + 1)
    assert fetched == (K + 1) * LINES
    one = np.zeros(48, np.uint64)
    one[:4] = O.canon_to_mont_array([1]).reshape(4)
    assert np.array_equal(got, one)
