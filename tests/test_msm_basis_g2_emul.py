"""The bodies of the fixed-basis MSM (csrc/msm_basis.h: table build, the prefetch-shaped run
sum by mixed additions; msm.h, msm_group.h; curve.h jac_add_mixed) compiled for the host over
Fq2 inside the whole pipeline in plain loops (tests/native/msm_basis_g2_emul.cpp: recoding over
the zero flags, sort by key, accumulation out of the lane-half table, chunks and folds at a
forced cap, the collapse of the windows, the two-window reduction, the finish), against the
oracle bit for bit on the normalized image.  No device: the kernels are thin wrappers over the
same bodies.  Rows 2 and 23 of the pool are on-curve points outside the order-r subgroup."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_basis_g2_cases as C
from tests.native import msmbasisg2emul as E

NBASES = [1, 2, 3, 17, 65]
WINDOWS = [2, 5, 11]      # 11: a top window of one scalar bit, the most replicas; 2: of zero bits
CAPS = [E.UNSPLIT, 4, 1]  # 1: every entry its own chunk, two fold levels and more on the longer runs
NMAX = 65


@pytest.fixture(scope="module")
def pool():
    """NMAX bases, scalars and the oracle's products, computed once."""
    p = C.g2_points(NMAX, 9201)
    p[2] = C.off_subgroup_point(0x7157)
    p[C.OFF_AT] = C.off_subgroup_point(0x7158)
    kv, k = O.random_scalars(NMAX, seed=9202, lo=0)
    prod = O.g2_mul(p, k, nthreads=C.NT)
    for a in (p, k, prod):
        a.setflags(write=False)
    return {"p": p, "k": k, "kv": [int(v) for v in kv], "prod": prod}


def _canon(k):
    return [int(v) for v in O.mont_array_to_canon(np.ascontiguousarray(k).reshape(-1), O.FR)]


def test_the_planted_off_subgroup_bases_are_what_they_claim(pool):
    """A check of the test data alone: on the twist, and [r] q != 0 ((r - 1) q + q by the oracle)."""
    from tests import group_exceptional_cases as X
    for at in (2, C.OFF_AT):
        q = pool["p"][at:at + 1]
        assert X.model_on_curve(X.model_point(q[0]))
        rq = O.g2_add(O.g2_mul(q, C.fr([C.R - 1]), nthreads=1), q)
        assert rq[0, 16:24].any()                          # not the zero point: outside the order-r subgroup
    g = pool["p"][5:6]                                    # and a base of the subgroup is sent to zero
    assert not O.g2_add(O.g2_mul(g, C.fr([C.R - 1]), nthreads=1), g)[0, 16:24].any()


def test_the_default_width():
    """msm_basis_auto_window_g2: the table of DESIGN.md 8f, pinned on both sides of every step."""
    auto = E.lib().msm_basis_g2_emul_auto_window
    for nb, c in ((1, 9), (2047, 9), (2048, 11), (32767, 11), (32768, 12), (92681, 12), (92682, 14), (741454, 14),
                  (741455, 15), (1 << 20, 15), (1 << 26, 15)):
        assert auto(nb) == c, (nb, c)


@pytest.mark.parametrize("c", WINDOWS)
def test_table_entries_against_the_oracle(pool, c):
    nb = 5
    bases = pool["p"][:nb].copy()
    bases[3, 16:24] = 0                                   # a zero base under a real x, y
    tab, flags = E.table(bases, c)
    assert list(flags) == [0, 0, 0, 1, 0] and not tab[:, 3].any()
    nw = 254 // c + 1
    assert tab.shape == (nw, nb, 16)
    for w in (0, 1, nw // 2, nw - 1):
        lo = c * w // 2                                   # 2^(c w) may exceed r, and base 2 is outside the subgroup:
        half = O.g2_mul(bases, C.fr([1 << lo] * nb), nthreads=C.NT)   # two multiplications by integers below r
        want = O.g2_normalize(O.g2_mul(half, C.fr([1 << (c * w - lo)] * nb), nthreads=C.NT))
        for b in (0, 1, 2, 4):                            # 2: the off-subgroup base
            assert want[b, 16:24].any() and np.array_equal(tab[w, b], want[b, :16]), (w, b)


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("nbases", NBASES)
def test_sweep(pool, nbases, c):
    bases = pool["p"][:nbases]
    for n in sorted({nbases, nbases // 2}):               # the whole basis and a proper prefix
        want = C.expect_from_products(pool["prod"][:n])
        for cap in CAPS:
            got, st = E.msm(bases, pool["kv"][:n], c, cap)
            assert np.array_equal(got, want), (n, cap)
            assert (st["levels"] > 0) == (cap != E.UNSPLIT and n > cap), (n, cap, st)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("c", WINDOWS)
def test_planted_rows(pool, c, cap):
    p, k = C.planted(pool["p"], pool["k"], c)
    want = C.expect(p, k)
    got, _ = E.msm(p, _canon(k), c, cap)
    assert np.array_equal(got, want)
    n = 24                                                # the planted rows and the off-subgroup base, as a prefix
    got, _ = E.msm(p, _canon(k[:n]), c, cap)
    assert np.array_equal(got, C.expect(p[:n], k[:n]))


@pytest.mark.parametrize("c", WINDOWS)
def test_all_scalars_equal(pool, c):
    """One bucket per window holds every term: long keys at the forced cap, two fold levels."""
    n = NMAX
    k = np.ascontiguousarray(np.broadcast_to(pool["k"][5], (n, 4)))
    want = C.expect(pool["p"], k)
    for cap, levels in ((E.UNSPLIT, 0), (4, 1), (1, 2)):
        got, st = E.msm(pool["p"], [pool["kv"][5]] * n, c, cap)
        assert np.array_equal(got, want), cap
        assert st["levels"] == levels and (st["long"] > 0) == (levels > 0), (cap, st)


def test_cancelling_pairs_and_the_zero_sum(pool):
    z = C.zero()
    kv = 0x1f2e3d4c5b6a79880123456789abcdef
    p = np.stack([pool["p"][7], pool["p"][7], pool["p"][9], O.g2_neg(pool["p"][9:10])[0]])
    for c in WINDOWS:
        got, _ = E.msm(p, [kv, C.R - kv, 5, 5], c)
        assert np.array_equal(got, z), c
        assert np.array_equal(E.msm(p, [0, 0, 0, 0], c)[0], z)
        assert np.array_equal(E.msm(p, [], c)[0], z)      # n == 0
