"""The group-law bodies of the bucket MSM (csrc/msm_group.h: per-bucket sum,
per-segment reduction, Horner, finish) compiled for the host over Fq2 and over Fq,
inside the whole pipeline in plain loops (tests/native/msm_g2_emul.cpp), against the
oracle bit for bit on the normalized image.  No device: the G2 kernels are thin
wrappers over the same bodies."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_g2_cases as C
from tests.native import msmg2emul

WINDOWS = [2, 3, 5, 10]  # 2 and 10 have top-window replicas (254 - c * floor(254 / c) < c - 1)
SIZES = [0, 1, 2, 3, 33, 65]
NMAX = 65


@pytest.fixture(scope="module")
def pool():
    """NMAX points of each group, scalars and the oracle's products, computed once."""
    q = C.g2_points(NMAX, 7101)
    _, s = O.random_scalars(NMAX, 7101)
    p = O.g1_mul(O.g1_one(), s, C.NT)
    kv, k = O.random_scalars(NMAX, seed=7102, lo=0)
    out = {"g2": q, "g1": p, "k": k, "kv": kv,
           "prod_g2": O.g2_mul(q, k, nthreads=C.NT), "prod_g1": O.g1_mul(p, k, nthreads=C.NT)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _expect_g1(prod):
    z = np.zeros(12, np.uint64)
    z[4:8] = O.canon_to_mont_array([1]).reshape(4)
    a = prod.reshape(-1, 12).copy()
    if a.shape[0] == 0:
        return z
    while a.shape[0] > 1:
        h = (a.shape[0] + 1) // 2
        m = a.shape[0] - h
        a[:m] = O.g1_add(a[:m], a[h:])
        a = a[:h]
    r = O.g1_normalize(a)[0]
    return r if r[8:12].any() else z


def test_the_replica_claim_and_the_segment_length():
    for c, has in ((2, True), (3, False), (5, False), (10, True)):
        top = 254 - c * (254 // c)
        assert ((c - 1) - top > 0) == has
    assert msmg2emul.lib().msm_g2_emul_segment() == 16


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_g2_pipeline(pool, c, n):
    got = msmg2emul.msm("g2", pool["g2"][:n], pool["kv"][:n], c)
    assert np.array_equal(got, C.expect_from_products(pool["prod_g2"][:n]))


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_g1_pipeline(pool, c, n):
    got = msmg2emul.msm("g1", pool["g1"][:n], pool["kv"][:n], c)
    assert np.array_equal(got, _expect_g1(pool["prod_g1"][:n]))


@pytest.fixture(scope="module")
def planted(pool):
    p, k = C.plant(pool["g2"][:NMAX], pool["k"][:NMAX], lambda nw: (1, nw - 1))
    return p, O.mont_array_to_canon(k.reshape(-1), O.FR), C.expect(p, k)


@pytest.mark.parametrize("c", WINDOWS)
def test_g2_planted_cases(planted, c):
    p, kv, want = planted
    assert np.array_equal(msmg2emul.msm("g2", p, kv, c), want)


def test_g2_cancelling_and_zero_sums(pool):
    q = pool["g2"]
    kv = 0x1f2e3d4c5b6a79880123456789abcdef
    for c in WINDOWS:
        assert np.array_equal(msmg2emul.msm("g2", np.stack([q[17], q[17]]), [kv, C.R - kv], c), C.zero())
        assert np.array_equal(msmg2emul.msm("g2", q[:5], [0] * 5, c), C.zero())
