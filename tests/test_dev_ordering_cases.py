"""tests/dev_ordering_cases.py on the oracle alone (no GPU): every chain's expected value
differs from the answer for the valid placeholder V0 that the consumer would read if it ran
before its producer, the placeholders are what they claim to be, and the planted control
arrays have the shapes the GPU test relies on."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import dev_ordering_cases as D


@pytest.fixture(scope="module")
def cases():
    return D.cases()


@pytest.mark.parametrize("chain,want,v0", D.V0_PAIRS)
def test_expected_value_differs_from_the_v0_answer(cases, chain, want, v0):
    w, v = cases[chain][want], cases[chain][v0]
    assert w.shape == v.shape and w.any() and v.any()
    assert not np.array_equal(w, v)


def test_every_row_that_depends_on_the_producer_differs(cases):
    """A product or a power takes one input from the producer in every row; the per-pair
    chains only in row 0."""
    for chain, want, v0 in (("many_products", "want", "v0"), ("prepared_products", "want", "v0"), ("pow", "want7", "v0_7"),
                            ("pow", "want5", "v0_5"), ("pow", "want_prepared", "v0_7")):
        w, v = cases[chain][want], cases[chain][v0]
        assert (w != v).any(axis=1).all(), chain
    for chain, want, v0 in (("msm_pairs", "want_many", "v0_many"), ("g2msm_pairs", "want", "v0")):
        w, v = cases[chain][want], cases[chain][v0]
        assert (w[0] != v[0]).any() and np.array_equal(w[1:], v[1:]), chain


def test_placeholders_are_valid_values(cases):
    one = O.canon_to_mont_array([1]).reshape(4)
    g1, g2, gt = D.g1_gen(), D.g2_gen(), D.gt_one()
    assert np.array_equal(g1[8:12], one) and O.g1_eq(g1[None, :], O.g1_normalize(g1[None, :]))[0]
    assert np.array_equal(g2[16:20], one) and not g2[20:24].any()
    assert np.array_equal(gt[:4], one) and not gt[4:].any()
    # Gt::one() to any power is itself: the V0 answer of every power chain
    assert np.array_equal(cases["pow"]["v0_7"], np.tile(gt, (7, 1)))
    # the placeholder is not the right value anywhere
    assert not np.array_equal(cases["msm_pairs"]["sum"], g1) and not np.array_equal(cases["g2msm_pairs"]["sum"], g2)
    assert (cases["many_products"]["sums"] != g1).any(axis=1).all()
    assert (cases["prepared_products"]["sums"] != g1).any(axis=1).all()
    assert (cases["pow"]["gt7"] != gt).any(axis=1).all() and (cases["pow"]["prod5"] != gt).any(axis=1).all()


def test_msm_sums_are_normalized_and_agree_across_helpers(cases):
    one = O.canon_to_mont_array([1]).reshape(4)
    m = cases["msm_pairs"]
    assert np.array_equal(m["sum"][8:12], one)
    # the single MSM's value from the segmented helper too (one segment of all 257 terms)
    from tests import msm_many_cases as M
    assert np.array_equal(M.expect(m["p"], m["k"], M.offsets_of([257]))[0], m["sum"])
    assert np.array_equal(cases["regrow"]["msm6"], M.expect(m["p"][:6], m["k"][:6], M.offsets_of([6]))[0])


def test_hand_off_control_arrays(cases):
    h = cases["handoff"]
    assert len(h["off_x"]) != len(h["off_y"]) and int(h["off_x"][-1]) == 12 and int(h["off_y"][-1]) == 17
    assert set(h["off_x"][1:-1]).isdisjoint(h["off_y"][1:-1])            # other cut points
    assert len(h["qidx_x"]) == 12 and len(h["qidx_y"]) == 17
    assert int((h["qidx_x"] == D.FRESH).sum()) == len(h["fresh_x"])
    assert int((h["qidx_y"] == D.FRESH).sum()) == len(h["fresh_y"])
    assert not np.array_equal(h["qidx_x"], h["qidx_y"][:12])
    # A computed with B's arrays would not give A's rows
    assert not np.array_equal(h["want_x"], h["want_y"][:4]) and not np.array_equal(h["want_px"], h["want_py"][:4])
    assert not np.array_equal(h["want_mx"], h["want_my"][:3])
    assert int(h["moff_x"][-1]) == 9 and int(h["moff_y"][-1]) == 15


def test_sticky_outcome_rows(cases):
    p = cases["prepared"]
    assert int(p["bad_idx"][3]) == len(p["q"]) and not p["bad_want"][3].any()
    keep = [i for i in range(7) if i != 3]
    assert np.array_equal(p["bad_want"][keep], p["want"][keep])
