"""The bodies of the fixed-basis MSM (csrc/msm_basis.h: table build, the prefetch-shaped run
sum by mixed additions; msm.h, msm_group.h; curve.h jac_add_mixed) compiled for the host over
Fq inside the whole pipeline in plain loops (tests/native/msm_basis_emul.cpp: recoding over the
zero flags, sort by key, accumulation, chunks and folds at a forced cap, the collapse of the
windows, the two-window reduction, the finish), against the oracle bit for bit on the
normalized image.  No device: the kernels are thin wrappers over the same bodies."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_basis_cases as C
from tests.native import msmbasisemul as E

NBASES = [1, 2, 3, 17, 65]
WINDOWS = [2, 5, 11]      # 11: a top window of one scalar bit, the most replicas; 2: of zero bits
CAPS = [E.UNSPLIT, 4]
NMAX = 65


@pytest.fixture(scope="module")
def pool():
    """NMAX bases, scalars and the oracle's products, computed once."""
    p = C.g1_points(NMAX, 9101)
    kv, k = O.random_scalars(NMAX, seed=9102, lo=0)
    prod = O.g1_mul(p, k, nthreads=C.NT)
    for a in (p, k, prod):
        a.setflags(write=False)
    return {"p": p, "k": k, "kv": [int(v) for v in kv], "prod": prod}


def _canon(k):
    return [int(v) for v in O.mont_array_to_canon(np.ascontiguousarray(k).reshape(-1), O.FR)]


def test_entry_counts_and_the_default_width():
    L = E.lib()
    ent, auto = L.msm_basis_emul_entries, L.msm_basis_emul_auto_window
    assert ent(1, 16) == 16 and ent(1 << 20, 16) == 16 << 20 and ent(5, 2) == 5 * 128 and ent(3, 11) == 3 * 24
    for nb in (1, 4099, 1 << 16, 1 << 18, 1 << 20, 1 << 26):
        assert 2 <= auto(nb) <= 16
        assert ent(nb, 0) == ent(nb, auto(nb)) > 0        # 0: the default width
    for nb, c in ((0, 8), (1, 1), (1, 17), (1, -3), ((1 << 26) + 1, 16), (1 << 60, 16)):
        assert ent(nb, c) == 0, (nb, c)
    lim = (2 ** 31 - 1) // 128                            # nbases * W(2) up to 2^31 - 1
    assert ent(lim, 2) == lim * 128 and ent(lim + 1, 2) == 0
    assert ent(1 << 26, 9) == 29 << 26 and ent(1 << 26, 8) == 0   # W(8) = 32: 2^31 entries, one too many


@pytest.mark.parametrize("c", WINDOWS)
def test_table_entries_against_the_oracle(pool, c):
    nb = 5
    bases = pool["p"][:nb].copy()
    bases[3, 8:12] = 0                                    # a zero base under a real x, y
    tab, flags = E.table(bases, c)
    assert list(flags) == [0, 0, 0, 1, 0] and not tab[:, 3].any()
    nw = 254 // c + 1
    assert tab.shape == (nw, nb, 8)
    for w in (0, 1, nw // 2, nw - 1):
        want = O.g1_normalize(O.g1_mul(bases, C.fr([1 << (c * w)] * nb), nthreads=C.NT))
        for b in (0, 1, 2, 4):
            assert np.array_equal(tab[w, b], want[b, :8]), (w, b)


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("nbases", NBASES)
def test_sweep(pool, nbases, c):
    bases = pool["p"][:nbases]
    for n in sorted({nbases, nbases // 2}):               # the whole basis and a proper prefix
        want = C.expect_from_products(pool["prod"][:n])
        for cap in CAPS:
            got, st = E.msm(bases, pool["kv"][:n], c, cap)
            assert np.array_equal(got, want), (n, cap)
            assert (st["levels"] > 0) == (cap == 4 and n > 4), (n, cap, st)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("c", WINDOWS)
def test_planted_rows(pool, c, cap):
    p, k = C.planted(pool["p"], pool["k"], c)
    want = C.expect(p, k)
    got, _ = E.msm(p, _canon(k), c, cap)
    assert np.array_equal(got, want)
    n = 24                                                # the planted rows alone, as a prefix
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
    p = np.stack([pool["p"][7], pool["p"][7], pool["p"][9], O.g1_neg(pool["p"][9:10])[0]])
    for c in WINDOWS:
        got, _ = E.msm(p, [kv, C.R - kv, 5, 5], c)
        assert np.array_equal(got, z), c
        assert np.array_equal(E.msm(p, [0, 0, 0, 0], c)[0], z)
        assert np.array_equal(E.msm(p, [], c)[0], z)      # n == 0
