"""The loop body of k_pairing_prepared (pairing.h miller_prepared) on the host: the Miller
loop over the unscaled lines of an affine Q, as a bn_g2_prepared table holds them, in both
forms (tests/native/prepared_emul.cpp, the one-lane layout, with the fold-bound checks of
BN_HOST_CHECKS, which abort the process).

  - Miller form (ell_0 as stored, ell_vw * y_P, ell_vv * x_P): for 3 random affine Q and P in
    {random affine, the generator} the value is the oracle's G2Precomp::miller_loop over the
    oracle's own precompute of Q, bit for bit;
  - Gt form (ell_0 * Z^3, ell_vw * Y, ell_vv * X Z on the Jacobian P): at z != one the Miller
    value differs from that one (by a power of Z), at z == one it is the same; either way its
    final exponentiation is the oracle's pairing of the pair, bit for bit.
The kernel around this body is checked end to end by tests/test_gpu_prepared.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.native import preparedemul

NQ = 3
LINES = 87


@pytest.fixture(scope="module")
def data():
    p, q, _, _ = O.random_pairs(NQ, seed=7301, nthreads=4)
    pa, rp = O.g1_to_affine(p)
    qa, rq = O.g2_to_affine(q)
    assert not any(rp) and not any(rq)
    one = O.canon_to_mont_array([1]).reshape(4)
    assert not any(np.array_equal(p[k, 8:12], one) for k in range(NQ))   # Jacobian, z != one
    pn = O.g1_normalize(p)                                               # the same points at z == one
    assert all(np.array_equal(pn[k, 8:12], one) for k in range(NQ))
    gen = O.g1_one()
    want = {}
    for j in range(NQ):
        coeffs = O.g2_precompute(qa[j])
        want[j, "rand"] = O.miller_loop(coeffs, pa[j, :4], pa[j, 4:])
        want[j, "gen"] = O.miller_loop(coeffs, gen[0:4], gen[4:8])
    for a in (p, q, pa, qa, pn, gen):
        a.setflags(write=False)
    return {"p": p, "q": q, "pa": pa, "qa": qa, "pn": pn, "gen": gen, "want": want}


@pytest.mark.parametrize("which", ["rand", "gen"])
@pytest.mark.parametrize("j", range(NQ))
def test_miller_form_is_the_references_miller_loop(data, j, which):
    xy = data["pa"][j] if which == "rand" else data["gen"][:8]
    got, fetched = preparedemul.miller_prepared(data["qa"][j], xy, gt_form=False)
    assert fetched == LINES
    assert np.array_equal(got, data["want"][j, which])


@pytest.mark.parametrize("j", range(NQ))
def test_gt_form_at_jacobian_p_gives_the_pairing(data, j):
    got, fetched = preparedemul.miller_prepared(data["qa"][j], data["p"][j], gt_form=True)
    assert fetched == LINES
    assert not np.array_equal(got, data["want"][j, "rand"])   # off by a power of Z before the exponentiation
    out, _ = O.final_exponentiation(got)
    want = O.pairing_many(data["p"][j], data["q"][j])
    assert np.array_equal(out[0], want[0])


@pytest.mark.parametrize("j", range(NQ))
def test_gt_form_at_z_one_is_the_miller_value_itself(data, j):
    got, _ = preparedemul.miller_prepared(data["qa"][j], data["pn"][j], gt_form=True)
    assert np.array_equal(got, data["want"][j, "rand"])      # Z = one: every factor is one
    out, _ = O.final_exponentiation(got)
    assert np.array_equal(out[0], O.pairing_many(data["pn"][j], data["q"][j])[0])
    assert np.array_equal(out[0], O.pairing_many(data["p"][j], data["q"][j])[0])


def test_gt_form_with_the_generator(data):
    got, _ = preparedemul.miller_prepared(data["qa"][0], data["gen"], gt_form=True)
    assert np.array_equal(got, data["want"][0, "gen"])
    out, _ = O.final_exponentiation(got)
    assert np.array_equal(out[0], O.pairing_many(data["gen"], data["q"][0])[0])
