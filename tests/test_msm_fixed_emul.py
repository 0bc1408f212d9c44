"""The bodies of the prepared-bases MSM (csrc/msm_fixed.h: table build, per-lane lookup
sums; curve.h jac_add_mixed) compiled for the host over Fq inside the whole pipeline in
plain loops (tests/native/msm_fixed_emul.cpp), against the oracle bit for bit on the
normalized images.  No device: the kernels are thin wrappers over the same bodies."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_prepared_cases as C
from tests.native import msmfixedemul

KS = [1, 2, 3, 5]
WINDOWS = [2, 5, 8]
LANES = [1, 2, 8]
M = 6


@pytest.fixture(scope="module")
def pool():
    """Five bases, M rows of five scalars and the oracle's products, computed once."""
    bases = C.g1_points(5, 8101)
    kv, k = O.random_scalars(M * 5, seed=8102, lo=0)
    k = k.reshape(M, 5, 4)
    out = {"bases": bases, "k": k, "kv": np.array(kv, dtype=object).reshape(M, 5), "prod": C.products(bases, k)}
    for a in (bases, k, out["prod"]):
        a.setflags(write=False)
    return out


def test_entry_counts_and_the_lane_rule():
    L = msmfixedemul.lib()
    assert L.msm_fixed_emul_entries(1, 8) == 32 * 128
    assert L.msm_fixed_emul_entries(16, 8) == 16 * 32 * 128
    assert L.msm_fixed_emul_entries(3, 0) == L.msm_fixed_emul_entries(3, 10)  # 0: the default width
    assert L.msm_fixed_emul_entries(1, 2) == 128 * 2 and L.msm_fixed_emul_entries(1, 16) == 16 * (1 << 15)
    for k, c in ((0, 8), (1, 1), (1, 17), (1 << 20, 8), (4096, 16)):
        assert L.msm_fixed_emul_entries(k, c) == 0, (k, c)
    assert L.msm_fixed_emul_entries((1 << 31) // 4096 - 1, 8) > 0
    # the smallest power of two with m * L >= 2^17 (2^19 from 832 pairs on), at most 64 and at
    # most a quarter of the k * W(c) pairs
    auto = L.msm_fixed_emul_auto_lanes
    assert auto(1 << 17, 16, 8) == 1 and auto(1 << 16, 16, 8) == 2 and auto(1 << 14, 16, 8) == 8
    assert auto(1 << 10, 16, 8) == 64
    assert auto(1 << 16, 64, 10) == 8 and auto(1 << 19, 64, 10) == 1 and auto(1 << 10, 64, 10) == 64
    assert auto(1 << 16, 32, 10) == 8 and auto(1 << 16, 31, 10) == 2    # 832 and 806 pairs
    assert auto(1, 1, 8) == 8      # W(8) = 32 pairs
    assert auto(1, 1, 16) == 4     # W(16) = 16
    assert auto(1, 3, 13) == 8     # 60 pairs
    assert auto(1, 1, 2) == 32 and auto(0, 5, 8) == 32


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("k", KS)
def test_sweep(pool, k, c):
    want = C.expect_from_products(pool["prod"][:, :k])
    rows = [list(r[:k]) for r in pool["kv"]]
    for lanes in LANES:
        got = msmfixedemul.msm_many(pool["bases"][:k], rows, c, lanes)
        assert np.array_equal(got, want), lanes


@pytest.mark.parametrize("c", WINDOWS)
def test_planted_rows(pool, c):
    rows = C.planted_values(c)
    k = C.fr([v for row in rows for v in row]).reshape(-1, 5, 4)
    for zero_form, lanes in ((0, 2), (1, 8)):
        bases = C.planted_bases(pool["bases"], zero_form)
        want = C.expect(bases, k)
        assert np.array_equal(want[0], C.zero()) and np.array_equal(want[2], C.zero())
        assert np.array_equal(want[4], C.zero())
        assert np.array_equal(want[1], O.g1_normalize(O.g1_add(bases[0:1], bases[0:1]))[0])
        got = msmfixedemul.msm_many(bases, rows, c, lanes)
        assert np.array_equal(got, want), (zero_form, lanes)


def test_normalized_and_jacobian_bases_give_the_same_bytes(pool):
    bases = pool["bases"][:3]
    norm = O.g1_normalize(bases)
    one = O.canon_to_mont_array([1]).reshape(4)
    assert all(np.array_equal(r[8:12], one) for r in norm) and not np.array_equal(bases[0, 8:12], one)
    rows = [list(r[:3]) for r in pool["kv"]]
    want = C.expect_from_products(pool["prod"][:, :3])
    for b in (bases, norm):
        assert np.array_equal(msmfixedemul.msm_many(b, rows, 5, 2), want)


def _same_point(a, b):
    na, nb = O.g1_normalize(a.reshape(1, 12))[0], O.g1_normalize(b.reshape(1, 12))[0]
    za, zb = not na[8:12].any(), not nb[8:12].any()
    return (za and zb) or (not za and not zb and np.array_equal(na, nb))


def test_jac_add_mixed_against_the_oracle(pool):
    """As points (both sides normalized): its Jacobian image need not be the general formula's."""
    acc, ent = pool["bases"][0], O.g1_normalize(pool["bases"][1:2])[0]
    neg_ent = O.g1_normalize(O.g1_neg(ent.reshape(1, 12)))[0]
    z2 = pool["bases"][3].copy()
    z2[8:12] = 0
    cases = {"random": acc, "zero": C.zero(), "zero with foreign x, y": z2,
             "equal": pool["bases"][1], "equal, normalized": ent,
             "minus": O.g1_neg(pool["bases"][1:2])[0], "minus, normalized": neg_ent}
    for name, a in cases.items():
        for neg in (False, True):
            e = neg_ent if neg else ent
            want = O.g1_add(a.reshape(1, 12), e.reshape(1, 12))[0]
            got = msmfixedemul.add_mixed(a, ent[:8], neg)
            assert _same_point(got, want), (name, neg)
    # the shortcuts give what they should: zero + entry is the entry's own image, P + (-P) a zero point
    assert np.array_equal(msmfixedemul.add_mixed(C.zero(), ent[:8]), ent)
    assert not msmfixedemul.add_mixed(neg_ent, ent[:8])[8:12].any()
    assert _same_point(msmfixedemul.add_mixed(ent, ent[:8]), O.g1_add(ent.reshape(1, 12), ent.reshape(1, 12))[0])
