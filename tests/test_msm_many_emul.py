"""The bodies of bn_g1_msm_many's packed path (csrc/msm_many.h: digits and multiples per
term, the units' shared-doubling sums, the segments' finish) compiled for the host over Fq
inside the whole pipeline in plain loops, with the plan of csrc/msm_many_plan.h
(tests/native/msm_many_emul.cpp), against the oracle bit for bit on the normalized images.
No device: the kernels are thin wrappers over the same bodies.  Every row of every case is
compared."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_many_cases as M
from tests.native import msmmanyemul

WINDOWS = [2, 4, 5, 8]
UNITS = [1, 2, 16]
LENGTHS = [0, 1, 2, 3, 17, 0, 5]


@pytest.fixture(scope="module")
def pool():
    """The ragged call's points, scalars and expected rows, and five points for the planted
    segments, computed once."""
    n = sum(LENGTHS)
    pts = M.g1_points(n, 8301)
    kv, k = O.random_scalars(n, seed=8302, lo=0)
    off = M.offsets_of(LENGTHS)
    want = M.expect(pts, k, off)
    for a in (pts, k, want):
        a.setflags(write=False)
    return {"p": pts, "kv": [int(v) for v in kv], "off": off, "want": want, "five": M.g1_points(5, 8303)}


def test_digit_bytes():
    L = msmmanyemul.lib()
    for d in range(-127, 129):     # every digit of every width up to 8
        assert L.msm_many_emul_digit_roundtrip(d) == d


@pytest.mark.parametrize("c", WINDOWS)
def test_ragged(pool, c):
    assert np.array_equal(pool["want"][0], M.zero()) and np.array_equal(pool["want"][5], M.zero())
    for unit in UNITS + [0]:
        got = msmmanyemul.msm_many(pool["p"], pool["kv"], pool["off"], c, unit)
        assert np.array_equal(got, pool["want"]), unit
    # several launch sets, and automatic units above 1 (two lanes wanted of 17 terms)
    assert np.array_equal(msmmanyemul.msm_many(pool["p"], pool["kv"], pool["off"], c, 2, chunk=4), pool["want"])
    assert np.array_equal(msmmanyemul.msm_many(pool["p"], pool["kv"], pool["off"], c, 0, lanes=2), pool["want"])


@pytest.mark.parametrize("c", WINDOWS)
def test_planted_rows(pool, c):
    for zero_form in (0, 1):
        p, vals, off = M.planted(pool["five"], c, zero_form)
        want = M.expect(p, M.fr(vals), off)
        assert np.array_equal(want[0], M.zero()) and np.array_equal(want[2], M.zero())   # 0 scalars; B and -B
        assert np.array_equal(want[4], M.zero())                                          # the zero point alone
        assert np.array_equal(want[1], O.g1_normalize(O.g1_add(p[0:1], p[0:1]))[0])       # A + A
        for unit in UNITS:
            got = msmmanyemul.msm_many(p, vals, off, c, unit)
            bad = [j for j in range(len(want)) if not np.array_equal(got[j], want[j])]
            assert not bad, (zero_form, unit, bad)


def test_normalized_and_jacobian_points_give_the_same_bytes(pool):
    norm = O.g1_normalize(pool["p"])
    one = O.canon_to_mont_array([1]).reshape(4)
    assert all(np.array_equal(r[8:12], one) for r in norm) and not np.array_equal(pool["p"][0, 8:12], one)
    for pts in (pool["p"], norm):
        assert np.array_equal(msmmanyemul.msm_many(pts, pool["kv"], pool["off"], 4, 2), pool["want"])


def test_one_long_segment_in_many_units(pool):
    """27 terms as one segment: 27, 14 and 2 units of it, and the 64-unit cap untouched"""
    off = M.offsets_of([27])
    p, kv = pool["p"][:27], pool["kv"][:27]
    want = M.expect(p, M.fr(kv), off)
    for unit in (1, 2, 16):
        assert np.array_equal(msmmanyemul.msm_many(p, kv, off, 4, unit), want), unit
