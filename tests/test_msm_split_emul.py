"""The split of overlong bucket runs of the bucket MSM on the CPU
(tests/native/msm_split_emul.cpp).  (a) The plan of csrc/msm.h -- run cap, chunk and group
positions, levels, array bounds -- walked slot by slot over synthetic histograms as the
device's lanes walk it: every entry of a long run lies in exactly one chunk, the slots of
every level are disjoint and inside the reserved bound, every long key writes its bucket at
exactly one level, within the fold launches the host sizes from n alone.  (b) The whole
pipeline with the split in plain loops over Fq and Fq2 with csrc/msm_group.h's bodies,
against the oracle bit for bit.  No device: the kernels are thin wrappers over the same
plan and bodies."""
import math
import subprocess

import numpy as np
import pytest

from tests import msm_skew_cases as C
from tests.native import msmsplitemul as M

CAPS = [1, 3, 64]
WINDOWS = [2, 5]
NMAX = 257


def _ok(counts, L, n=None, slack=0):
    counts = np.asarray(counts, np.uint32)
    n = int(counts.max()) if n is None else n
    rc, info = M.plan_check(counts, L, n, int(counts.sum()) + slack)
    assert rc == 0, (rc, info, L, n)
    return info


def test_constants():
    L = M.lib()
    assert L.msm_split_emul_fan() == 32 and L.msm_split_emul_run_min() == 128
    # the most levels: 2^26 terms at L = 1
    assert L.msm_split_emul_levels(1 << 26, 1) == L.msm_split_emul_max_levels() == 6
    for n, cap, levels in ((64, 64, 0), (65, 64, 1), (64 * 32, 64, 1), (64 * 32 + 1, 64, 2), (1 << 18, 64, 3),
                           (33, 1, 2), (1025, 1, 3), (4099, 1, 3), (5, M.UNSPLIT, 0)):
        assert L.msm_split_emul_levels(n, cap) == levels, (n, cap)


@pytest.mark.parametrize("L", [1, 2, 3, 7, 64])
def test_plan_edge_counts(L):
    F = 32
    counts = [L, L + 1] + [L * F ** k + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    for cnt in counts:
        if cnt < 1 or cnt > 70000:     # the walk is slot by slot: L * F^3 stays for the small caps
            continue
        info = _ok([cnt], L)                                   # everything in one key
        m, want_levels = -(-cnt // L), 0
        while m > 1:                                           # ceil(log_F(chunks))
            m, want_levels = -(-m // F), want_levels + 1
        assert info[0] == (1 if cnt > L else 0)
        assert info[1] == want_levels and info[3] == want_levels, (cnt, info)
        _ok([cnt, 0, 0, 0], L)                                 # a long key at key 0
        _ok([0, 0, 0, cnt], L)                                 # and at key nkeys - 1
        _ok([cnt, 1, cnt, L, cnt + 1, 0, 2 * L + 1], L, slack=5)  # long and short alternating


@pytest.mark.parametrize("L", [1, 3, 64])
def test_plan_long_keys_finish_at_different_levels(L):
    counts = [L * 32 ** 2 + 1, L, L + 1, 0, L * 32 + 1, 2 * L, L * 32, 1]
    info = _ok(counts, L)
    assert info[0] == 5 and info[1] == 3 == info[3]


@pytest.mark.parametrize("seed", range(8))
def test_plan_random_histograms(seed):
    rng = np.random.default_rng(100 + seed)
    for L in (1, 2, 5, 64):
        nkeys = int(rng.integers(1, 200))
        counts = np.where(rng.random(nkeys) < 0.2, rng.integers(0, 50 * L + 2, nkeys), rng.integers(0, L + 2, nkeys))
        _ok(counts, L, n=int(counts.max()) + int(rng.integers(0, 3 * L)), slack=int(rng.integers(0, 100)))


def test_plan_level0_bound_is_tight_enough():
    """The documented workspace bound: at most 2 * nent / L level-0 slots."""
    L = M.lib()
    for nent, nkeys, cap in ((1 << 24, 1 << 19, 64), (4099 * 16, 1 << 19, 1), (1000, 8, 3)):
        assert L.msm_split_emul_level_slots(nent, nkeys, cap, 0) <= 2 * nent // cap
        assert L.msm_split_emul_level_slots(nent, nkeys, cap, 1) <= L.msm_split_emul_level_slots(nent, nkeys, cap, 0)


# the automatic window tables (capi_msm.hip MsmGroup<P>::auto_window): (first n, last n, c)
G1_ROWS = [(1, 6143, 10), (6144, 92681, 12), (92682, 370727, 14), (370728, 741454, 15), (741455, 1 << 26, 16)]
G2_ROWS = [(1, 1448, 10), (1449, 23170, 11), (23171, 46340, 12), (46341, 370727, 14), (370728, 741454, 15),
           (741455, 1 << 26, 16)]


def _poisson_tail(mean, cap):
    """P(X > cap), X Poisson(mean), summed from cap + 1 until the terms vanish."""
    k = cap + 1
    term = math.exp(-mean + k * math.log(mean) - math.lgamma(k + 1))
    total = 0.0
    while term > 1e-300 and k < cap + 2000:
        total += term
        k += 1
        term *= mean / k
    return total


@pytest.mark.parametrize("rows", [G1_ROWS, G2_ROWS], ids=["g1", "g2"])
def test_default_cap_does_not_split_uniform_scalars(rows):
    """Uniform scalars put Poisson-like counts of mean about n / 2^(c-1) into the keys of a
    full window, and 2^254 / r = 1.32 times that into the top window's, whose digits only
    reach r's top bits.  At every row of the window tables (its ends, and 2^20 and 2^21
    where c = 16 has the smallest means for its cap) the default cap leaves the expected
    number of long keys of a call below one, and a sampled histogram of all the call's
    keys, the top window's that much fuller, has none."""
    L = M.lib()
    rng = np.random.default_rng(2024)
    for lo, hi, c in rows:
        for n in sorted({lo, hi, min(max(lo, 1 << 20), hi), min(max(lo, 1 << 21), hi)}):
            cap = L.msm_split_emul_cap_default(n, c)
            mean = n / (1 << (c - 1))
            assert cap >= 128 and cap >= 2 * mean
            nkeys = (254 // c + 1) << (c - 1)
            ntop = 1 << (c - 1)
            top = mean * (1 << 254) / C.R
            expected = (nkeys - ntop) * _poisson_tail(mean, cap) + ntop * _poisson_tail(top, cap)
            assert expected < 1, (n, c, cap, expected)
            counts = np.concatenate([rng.poisson(mean, nkeys - ntop), rng.poisson(top, ntop)])
            assert int((counts > cap).sum()) == 0, (n, c, cap, int(counts.max()))


@pytest.fixture(scope="module")
def pool():
    out = {}
    for name in ("g1", "g2"):
        g = C.Group(name)
        pts = g.points(NMAX, 7301)
        from oracle import oracle as O
        kv, k = O.random_scalars(NMAX, seed=7302, lo=0)
        prod = g.mul(pts, k, C.NT)
        for a in (pts, k, prod):
            a.setflags(write=False)
        out[name] = (g, pts, k, prod)
    return out


def _canon(k):
    from oracle import oracle as O
    return O.mont_array_to_canon(np.ascontiguousarray(k).reshape(-1), O.FR)


@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("pattern", C.PATTERNS)
def test_pipeline_with_the_split(pool, group, pattern):
    g, pts, uni_k, uni_prod = pool[group]
    for n in (33, NMAX) if group == "g1" else (65,):
        p, k, want = C.case(g, pattern, pts[:n], uni_k[:n], uni_prod[:n])
        kv = _canon(k)
        for c in WINDOWS:
            base, nlong, _ = M.msm(group, p, kv, c, M.UNSPLIT)
            assert np.array_equal(base, want), (n, c, "unsplit")
            assert nlong == 0
            for cap in CAPS:
                got, nlong, levels = M.msm(group, p, kv, c, cap)
                assert np.array_equal(got, want), (n, c, cap)
                if cap < n // 6:
                    assert nlong > 0 and levels > 0, (n, c, cap)   # the case does reach the split


def test_pipeline_default_cap_and_uniform_scalars(pool):
    g, pts, k, prod = pool["g1"]
    want = g.image(g.tree(prod))
    for cap in (0, 1, 3):
        got, nlong, _ = M.msm("g1", pts, _canon(k), 5, cap)
        assert np.array_equal(got, want), cap
        assert (nlong > 0) == (cap in (1, 3))


def test_standalone_program_under_sanitizers():
    """The plan's integer code (csrc/msm.h) as a stand-alone program with its own main under
    AddressSanitizer and UBSan: the plan checks over generated histograms."""
    exe = M.build_main(sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
