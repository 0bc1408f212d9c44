"""The whole batched fixed-basis pipeline (bn_g1_msm_basis_many) in plain loops over the index
arithmetic the kernels use (csrc/msm_basis_many.h) and the bodies of msm.h, msm_group.h and
msm_basis.h compiled for the host (tests/native/msm_basis_many_emul.cpp), against the oracle
bit for bit on every row's normalized image, and against the single-vector emulation of the
same row.  The emulator's arrays have exactly the sizes the host plan allocates and record
the highest index each stage asked for.  No device: the kernels are thin wrappers over the
same bodies and the same positions."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import msm_basis_cases as C
from tests.native import msmbasisemul as E1
from tests.native import msmbasismanyemul as E

MS = [1, 2, 3, 5]
NBASES = [0, 1, 3, 17, 65]
WINDOWS = [2, 5, 11]
CAPS = [E.UNSPLIT, 4, 1]
NMAX = 65
MMAX = 5


@pytest.fixture(scope="module")
def pool():
    """NMAX bases, MMAX rows of scalars and the oracle's products of every (row, base),
    computed once and left unchanged."""
    p = C.g1_points(NMAX, 9301)
    kv, k = O.random_scalars(MMAX * NMAX, seed=9302, lo=0)
    k = k.reshape(MMAX, NMAX, 4)
    prod = np.stack([O.g1_mul(p, k[j], nthreads=C.NT) for j in range(MMAX)])
    for a in (p, k, prod):
        a.setflags(write=False)
    kv = [[int(v) for v in kv[j * NMAX:(j + 1) * NMAX]] for j in range(MMAX)]
    return {"p": p, "k": k, "kv": kv, "prod": prod}


def _canon(k):
    return [int(v) for v in O.mont_array_to_canon(np.ascontiguousarray(k).reshape(-1), O.FR)]


def _within(st):
    for a in E.ARRAYS:
        assert st["touched"][a] <= st["alloc"][a], (a, st)


def _sets(m, S):
    return (m + S - 1) // S


@pytest.mark.parametrize("c", WINDOWS)
@pytest.mark.parametrize("m", MS)
def test_sweep(pool, m, c):
    for nb in NBASES:
        for n in sorted({nb, nb // 2}):                   # the whole basis and a proper prefix
            bases = pool["p"][:max(nb, 1)]
            rows = [pool["kv"][j][:n] for j in range(m)]
            want = np.stack([C.expect_from_products(pool["prod"][j, :n]) for j in range(m)])
            sets = sorted({1, 2, m})
            # every cap with every set size; at c = 11 (24,576 keys per vector: the collapse and
            # the reduction dominate the emulation) every cap and every set size once
            combos = [(cap, f) for cap in CAPS for f in sets] if c != 11 else list(zip(CAPS, (sets * 3)[:3]))
            for cap, forced in combos:
                got, st = E.msm(bases, rows, n, c, cap, forced)
                assert np.array_equal(got, want), (nb, n, cap, forced)
                _within(st)
                if n:
                    S = min(forced, m)
                    assert st["S"] == S and st["sets"] == _sets(m, S), (st, forced)
                    assert (st["levels"] > 0) == (cap != E.UNSPLIT and n > cap), (n, cap, st)


@pytest.mark.parametrize("c", WINDOWS)
def test_default_set_takes_every_vector_at_once(pool, c):
    rows = [pool["kv"][j][:17] for j in range(5)]
    got, st = E.msm(pool["p"][:17], rows, 17, c)
    assert st["S"] == 5 and st["sets"] == 1
    for j in range(5):
        assert np.array_equal(got[j], C.expect_from_products(pool["prod"][j, :17]))
        assert np.array_equal(got[j], E1.msm(pool["p"][:17], rows[j], c)[0])      # the single form's bytes
    _within(st)


@pytest.mark.parametrize("forced", [1, 2, 3])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("c", WINDOWS)
def test_one_row_all_equal_among_random_rows(pool, c, cap, forced):
    """Long keys and fold levels in one vector only: ranks and long-key lists are per vector."""
    n = NMAX
    rows = [pool["kv"][0], [pool["kv"][1][5]] * n, pool["kv"][2]]
    want = [C.expect_from_products(pool["prod"][0]),
            C.expect(pool["p"], np.ascontiguousarray(np.broadcast_to(pool["k"][1, 5], (n, 4)))),
            C.expect_from_products(pool["prod"][2])]
    got, st = E.msm(pool["p"], rows, n, c, cap, forced)
    assert np.array_equal(got, np.stack(want))
    _within(st)
    if cap == E.UNSPLIT:
        assert st["long"] == [0, 0, 0] and st["levels"] == 0
    else:
        # every nonzero window of the repeated scalar below the top one is one run of n entries
        assert st["long"][1] > 0, st
        if c == 11 and cap == 4:                          # 65 uniform terms over 1,024 buckets: no run above 4
            assert st["long"][0] == 0 and st["long"][2] == 0, st
        assert st["levels"] == (1 if cap == 4 else 2)


@pytest.mark.parametrize("forced", [1, 2, 3])
@pytest.mark.parametrize("c", WINDOWS)
def test_zero_row_identical_rows_and_padding(pool, c, forced):
    n = 17
    pad = [(1 << 256) - 1 - i for i in range(3)]          # k_stride = n + 3: a pattern that must not be read
    rows = [pool["kv"][0][:n] + pad, [0] * n + pad, pool["kv"][1][:n] + pad, pool["kv"][1][:n] + pad[::-1]]
    for cap in (E.UNSPLIT, 4):
        got, st = E.msm(pool["p"][:n], rows, n, c, cap, forced)
        assert np.array_equal(got[0], C.expect_from_products(pool["prod"][0, :n]))
        assert np.array_equal(got[1], C.zero())           # the empty vector: (0, one, 0)
        assert np.array_equal(got[2], C.expect_from_products(pool["prod"][1, :n]))
        assert np.array_equal(got[3], got[2])
        _within(st)


@pytest.mark.parametrize("cap", [E.UNSPLIT, 4])
@pytest.mark.parametrize("c", WINDOWS)
def test_planted_rows_in_one_row(pool, c, cap):
    p, k = C.planted(pool["p"], pool["k"][3], c)
    rows = [_canon(pool["k"][0]), _canon(k), _canon(pool["k"][4])]
    got, st = E.msm(p, rows, NMAX, c, cap, 2)
    assert np.array_equal(got[1], C.expect(p, k))
    assert np.array_equal(got[0], C.expect(p, pool["k"][0])) and np.array_equal(got[2], C.expect(p, pool["k"][4]))
    _within(st)
    got, _ = E.msm(p, rows, 24, c, cap)                   # the planted rows alone, as a prefix
    assert np.array_equal(got[1], C.expect(p[:24], k[:24]))


def test_cancelling_pairs_in_one_row(pool):
    kv = 0x1f2e3d4c5b6a79880123456789abcdef
    p = np.stack([pool["p"][7], pool["p"][7], pool["p"][9], O.g1_neg(pool["p"][9:10])[0]])
    rows = [pool["kv"][0][:4], [kv, C.R - kv, 5, 5], [0, 0, 5, 5], pool["kv"][1][:4]]
    for c in WINDOWS:
        got, st = E.msm(p, rows, 4, c, 0, 3)
        assert np.array_equal(got[1], C.zero()) and np.array_equal(got[2], C.zero()), c   # B and -B, equal scalars
        assert np.array_equal(got[0], E1.msm(p, rows[0], c)[0]) and np.array_equal(got[3], E1.msm(p, rows[3], c)[0])
        _within(st)
    got, st = E.msm(p, [[], [], []], 0, 5)                # n == 0
    assert np.array_equal(got, np.stack([C.zero()] * 3))
