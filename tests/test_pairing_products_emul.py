"""The loop body of k_miller_products (pairing.h miller_product_scaled) on the host: per
digit one squaring of the product's accumulator, then the line of each of its pairs, over
lines from g2_precompute scaled by P as the producers store them
(tests/native/products_emul.cpp, the one-lane layout, with the fold-bound checks of
BN_HOST_CHECKS).

  - K = 1, 2, 3, 5 live pairs: the Miller value is the oracle's miller_loop_batch, bit for bit;
  - dead pairs (the line one in their place, as the kernel gives a pair whose flag is set):
    at the first, a middle and the last position and at every position, the final
    exponentiation of the value is the oracle's pairing_batch with those points zeroed;
  - the wave-uniform padding: iterating to K + 3 pairs, the extra ones taking the line one,
    gives the same words as iterating to K.
The kernel around this body is checked end to end by tests/test_gpu_pairing_products.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.native import productsemul

KMAX = 5
LINES = 87


@pytest.fixture(scope="module")
def pairs():
    p, q, _, _ = O.random_pairs(KMAX, seed=6101, nthreads=4)
    pa, rp = O.g1_to_affine(p)
    qa, rq = O.g2_to_affine(q)
    assert not any(rp) and not any(rq)
    for a in (p, q, pa, qa):
        a.setflags(write=False)
    return {"p": p, "q": q, "pa": pa, "qa": qa}


def _zeroed(pairs, k, dead):
    """The first k pairs with the points at `dead` made zero: G1 at even positions, G2 at odd."""
    p, q = pairs["p"][:k].copy(), pairs["q"][:k].copy()
    one = O.canon_to_mont_array([1]).reshape(4)
    for t in dead:
        if t % 2 == 0:
            p[t] = 0
            p[t, 4:8] = one         # G1::zero() = (0, one, 0)
        else:
            q[t] = 0
            q[t, 8:12] = one        # G2::zero() = (0, one, 0)
    return p, q


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_live_pairs_give_the_oracles_miller_value(pairs, k):
    got, fetched = productsemul.miller_product(pairs["pa"][:k], pairs["qa"][:k])
    rc, want = O.miller_loop_batch(pairs["q"][:k], pairs["p"][:k])
    assert rc == 0
    assert fetched == k * LINES
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dead", [(0,), (2,), (4,), (0, 4), (0, 1, 2, 3, 4)])
def test_dead_pairs_take_the_line_one(pairs, dead):
    k = KMAX
    flags = np.zeros(k, np.uint8)
    flags[list(dead)] = 1
    got, _ = productsemul.miller_product(pairs["pa"][:k], pairs["qa"][:k], dead=flags)
    out, _ = O.final_exponentiation(got)
    p, q = _zeroed(pairs, k, dead)
    want = O.pairing_batch(p, q)
    assert np.array_equal(out[0], want)
    live = [t for t in range(k) if t not in dead]
    if live:
        rc, ml = O.miller_loop_batch(pairs["q"][live], pairs["p"][live])
        assert rc == 0 and np.array_equal(got, ml)   # the line one leaves the value itself unchanged
    else:
        one = np.zeros(48, np.uint64)
        one[:4] = O.canon_to_mont_array([1]).reshape(4)
        assert np.array_equal(got, one) and np.array_equal(want, one)


@pytest.mark.parametrize("k", [0, 1, 3])
def test_padding_past_the_products_own_count_changes_nothing(pairs, k):
    base, f0 = productsemul.miller_product(pairs["pa"][:k], pairs["qa"][:k])
    padded, f1 = productsemul.miller_product(pairs["pa"][:k], pairs["qa"][:k], iterate=k + 3)
    assert f0 == k * LINES and f1 == (k + 3) * LINES   # the padded loop did run the extra pairs
    assert np.array_equal(padded, base)
    if k == 0:
        one = np.zeros(48, np.uint64)
        one[:4] = O.canon_to_mont_array([1]).reshape(4)
        assert np.array_equal(base, one)
