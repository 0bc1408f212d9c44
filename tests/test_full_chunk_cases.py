"""tests/full_chunk_cases.py on the oracle alone (no GPU): the period blocks hold the rows they
are meant to hold, those rows lie where a 2^18-element launch set needs them (by index
arithmetic), the comparison helpers find a wrong row, and the byte offsets that make 2^18 the
size to test follow from the engine's constants."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import full_chunk_cases as F

# Copied from the engine; a change there must bring someone to this file and to
# tests/test_gpu_full_chunk.py:
K_CHUNK = 1 << 18        # kernels.h:26       constexpr size_t kChunk
SLOT_WORDS = 108         # kernels.h:27       constexpr int kSlotWords (one Fq12: 12 Fq x 9 digits)
GT_POW_ENTRIES = 17      # kernels.h:31       constexpr int kGtPowEntries
FE_SLOTS = 32            # capi.hip:17        constexpr int kFeSlots
NUM_COEFFS = 87          # include/bn254mi.h  BN_NUM_COEFFS; kCoeffFq = BN_NUM_COEFFS * 6 (kernels.h:25)
PATH_LANES = 2           # kernels.h:19       constexpr int kPathLanes
RSRC_RECORDS = 0x7fffffff  # kernels.h:94     slot_rsrc's num_records


@pytest.fixture(scope="module")
def b():
    return F.blocks()


def _source_constant(path, pattern):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "paritytech-bn_amd", "csrc", path)) as fh:
        m = re.search(pattern, fh.read())
    assert m, (path, pattern)
    return m.group(1)


def test_constants_are_the_engines():
    assert _source_constant("kernels.h", r"constexpr size_t kChunk = size_t\(1\) << (\d+);") == "18"
    assert _source_constant("kernels.h", r"constexpr int kSlotWords = (\d+);") == str(SLOT_WORDS)
    assert _source_constant("kernels.h", r"constexpr int kGtPowEntries = (\d+);") == str(GT_POW_ENTRIES)
    assert _source_constant("kernels.h", r"constexpr int kPathLanes = (\d+);") == str(PATH_LANES)
    assert _source_constant("capi.hip", r"constexpr int kFeSlots = (\d+);") == str(FE_SLOTS)
    assert _source_constant("kernels.h", r"make_buffer_rsrc\(\(void\*\)base, 0, (0x[0-9a-f]+),") == hex(RSRC_RECORDS)
    assert F.CHUNK == K_CHUNK and F.N == K_CHUNK and F.N1 == K_CHUNK + 1 and F.WAVE * PATH_LANES == 64


def test_offsets_a_full_launch_set_reaches():
    """The offset facts behind the choice of 2^18 (and what 2^16, the largest launch set of the
    other parity tests, reaches)."""
    n = K_CHUNK
    slot_bytes = SLOT_WORDS * 4                                 # 432 per element and slot
    coeff_bytes = NUM_COEFFS * 6 * 9 * 4                        # 18,792 per pairing
    assert slot_bytes == 432 and coeff_bytes == 18792
    # the workspace of one launch set (capi.hip ws_bytes): coefficients, affine P and flags, slots
    ws = n * (coeff_bytes + PATH_LANES * (2 * 9 * 4 + 1) + FE_SLOTS * slot_bytes) + 64
    assert ws == 8588361792 and 8.5e9 < ws < 8.7e9       # what bn_workspace_bytes(1 << 18) returns
    # slot t starts at byte t * 432 * n: from t = 19 up at or beyond 2^31, slot 31 near 3.5e9, and
    # the whole slot region ends below 2^32
    start = [t * slot_bytes * n for t in range(FE_SLOTS + 1)]
    assert [t for t in range(FE_SLOTS) if start[t] >= 1 << 31] == list(range(19, FE_SLOTS))
    assert 3.5e9 < start[31] < 3.52e9 and start[FE_SLOTS] < 1 << 32
    # slot 31 crosses 2^31 only from about 160 k elements on: no smaller power of two gets there
    assert 31 * slot_bytes * (1 << 17) < 1 << 31 < 31 * slot_bytes * 161000
    # the line coefficients of a full set pass 2^32 bytes
    assert n * coeff_bytes > 1 << 32 and 4.9e9 < n * coeff_bytes < 5.0e9
    # k_gt_pow's window table: 32-bit byte offsets through a descriptor of 2^31 - 1 records; the top
    # entry (16) ends at about 1.92e9, inside it, and entry 15 -- the generic chain's top -- below
    table_end = GT_POW_ENTRIES * slot_bytes * n
    assert 1.92e9 < table_end < 1.93e9 and table_end < RSRC_RECORDS
    assert (GT_POW_ENTRIES + 3) * slot_bytes * n > RSRC_RECORDS   # three more entries would not fit
    # what the 2^16 tests reach: nothing near 2^31
    assert 31 * slot_bytes * (1 << 16) < 8.8e8 and (1 << 16) * coeff_bytes < 1 << 31


def test_tiling_and_placement_arithmetic():
    assert F.PERIOD == 251 and all(F.PERIOD % d for d in range(2, 16))      # prime
    assert K_CHUNK % F.PERIOD == 100
    # a row and the row any power-of-two distance away are different rows of the block
    assert all((1 << s) % F.PERIOD for s in range(64))
    assert F.index_of(K_CHUNK - 1) == 99 and F.index_of(K_CHUNK) == 100
    assert F.wave_indices(-1) == list(range(68, 100))
    assert F.wave_indices(-2) == list(range(36, 68))
    assert F.wave_indices(0) == list(range(32))
    last8 = [F.wave_indices(-w) for w in range(1, 9)]
    assert sorted(set(sum(last8, []))) == list(range(F.PERIOD))            # 256 rows: every block row
    blk = np.arange(F.PERIOD * 3, dtype=np.uint64).reshape(F.PERIOD, 3)
    t = F.tile(blk, 2 * F.PERIOD + 7)
    assert t.shape == (509, 3) and np.array_equal(t[F.PERIOD:2 * F.PERIOD], blk) and np.array_equal(t[502:], blk[:7])
    assert np.array_equal(F.tile(np.arange(F.PERIOD, dtype=np.uint8), 300)[251:], np.arange(49, dtype=np.uint8))


def test_the_comparison_finds_one_wrong_row():
    blk = np.arange(F.PERIOD * 4, dtype=np.uint64).reshape(F.PERIOD, 4)
    n = 5 * F.PERIOD + 100
    got = F.tile(blk, n)
    assert F.first_mismatch(got, blk) is None and F.count_mismatches(got, blk) == 0
    F.assert_tiled(got, blk, "unchanged")
    for row in (0, 250, 251, 777, n - 100, n - 1):      # whole periods and the tail
        bad = got.copy()
        bad[row, 3] ^= 1
        assert F.first_mismatch(bad, blk) == (row, row % F.PERIOD, row - K_CHUNK)
        assert F.count_mismatches(bad, blk) == 1
        with pytest.raises(AssertionError, match="row %d " % row):
            F.assert_tiled(bad, blk, "one bit")
    # a row that holds ANOTHER row of the block (an address off by a power of two) is found
    bad = got.copy()
    bad[600] = got[600 - 512]
    assert F.first_mismatch(bad, blk)[0] == 600
    # the column mask: rows outside it are not compared
    cols = np.ones(F.PERIOD, bool)
    cols[17] = False
    bad = got.copy()
    bad[17 + F.PERIOD] += 1
    bad[n - 83] += 1                                     # block row 17 in the tail
    assert F.index_of(n - 83) == 17 and F.first_mismatch(bad, blk, cols) is None
    assert F.count_mismatches(bad, blk) == 2
    # one-dimensional outputs (status bytes)
    st = np.arange(F.PERIOD, dtype=np.uint8)
    g = F.tile(st, n)
    g[300] ^= 1
    assert F.first_mismatch(g, st)[0] == 300


def test_pair_block(b):
    one = O.canon_to_mont_array([1])
    z1, z2 = b.p[:, 8:12], b.q[:, 16:24]
    jac = [r for r in range(F.PERIOD) if r != F.AFFINE_PAIR and r not in F.G1_ZERO + F.G2_ZERO]
    assert len(jac) == F.PERIOD - 5
    for r in jac:   # random Jacobian: z neither one nor zero, on both sides
        assert z1[r].any() and not np.array_equal(z1[r], one) and z2[r].any() and not np.array_equal(z2[r, :4], one)
    assert np.array_equal(z1[F.AFFINE_PAIR], one) and np.array_equal(z2[F.AFFINE_PAIR, :4], one)
    assert not z2[F.AFFINE_PAIR, 4:].any()
    for r in F.G1_ZERO:
        assert not z1[r].any() and z2[r].any() and np.array_equal(b.e[r], b.gt_one)
    for r in F.G2_ZERO:
        assert not z2[r].any() and z1[r].any() and np.array_equal(b.e[r], b.gt_one)
    # every other pairing is a value of its own, and the rows are distinct
    assert len({b.e[r].tobytes() for r in range(F.PERIOD)}) == F.PERIOD - 3
    assert not any(np.array_equal(b.e[r], b.gt_one) for r in jac)
    # a zero point in the chunk's last wave, and the one-element set behind a full one is a real pairing
    assert set(F.wave_indices(-1)) & set(F.G1_ZERO + F.G2_ZERO) and F.index_of(K_CHUNK) in jac
    # the Miller values: one for a zero point, and the oracle's final exponentiation leads to e
    for r in F.G1_ZERO + F.G2_ZERO:
        assert np.array_equal(b.ml[r], b.gt_one)
    fe, rcs = O.final_exponentiation(b.ml[:8])
    assert np.array_equal(fe, b.e[:8])


def _cyclotomic(x):
    """x^(p^4) * x == x^(p^2), x != 0 (kernels_gtpow.hip gt_pow_wave_cyclotomic)."""
    x = np.ascontiguousarray(x).reshape(1, 48)
    x2 = F._frob(x, 2)
    x4x = O.binary("orc_fq12_mul", F._frob(x2, 2), x, 48, 48, 48)
    return bool(x.any()) and np.array_equal(x4x, x2)


def test_fq12_block(b):
    member = [_cyclotomic(b.f[r]) for r in range(F.PERIOD)]
    assert len(F.MILLER) >= 2 and not b.f[F.ZERO_ROW].any()
    assert [r for r in range(F.PERIOD) if not member[r]] == sorted(F.MILLER + (F.ZERO_ROW,))
    for r in F.MILLER:
        assert b.f[r].any() and np.array_equal(b.f[r], b.ml[r])
    # final_exponentiation_many's block: Miller values, the zero row ok = 0 with a zero image
    assert not b.fe_in[F.ZERO_ROW].any() and not b.fe_out[F.ZERO_ROW].any()
    assert [r for r in range(F.PERIOD) if not b.fe_ok[r]] == [F.ZERO_ROW]
    assert all(b.fe_in[r].any() for r in range(F.PERIOD) if r != F.ZERO_ROW)
    # position at n = 2^18: among the last 8 waves a cyclotomic-only one (the last) and one holding
    # Miller values and the zero row (the one before it)
    assert all(member[r] for r in F.wave_indices(-1))
    assert set(F.MILLER) & set(F.wave_indices(-2)) and F.ZERO_ROW in F.wave_indices(-2)
    assert member[F.index_of(K_CHUNK)]                    # the one-element set: the signed chain
    # inv(0) = 0 in the oracle's answer, as BN_FQ12_INV states
    assert not b.fq12["inv"][F.ZERO_ROW].any()
    assert set(b.fq12) == {"mul", "sqr", "inv", "cyc_sqr", "exp_by_neg_z", "frob1", "frob2", "frob3"}


def test_scalar_block(b):
    k = b.k_vals
    assert np.array_equal(b.k, O.canon_to_mont_array(k, O.FR).reshape(-1, 4)) and all(0 <= v < O.R for v in k)
    assert {0, 1, O.R - 1} <= set(k) and set(F.RUNS) <= set(k)
    for r in F.TOP_BOOTH:
        assert max(abs(d) for d in F.booth_digits(k[r])) == 16
    signs = {d for r in F.TOP_BOOTH for d in F.booth_digits(k[r]) if abs(d) == 16}
    assert signs == {16, -16}                              # entry 16 as it is and conjugated
    for r in F.TOP_NIBBLE:
        assert 15 in F.nibbles(k[r])
    # position at n = 2^18: a top-digit scalar in the chunk's last 32 rows (its very last row),
    # in a cyclotomic-only wave, so the signed chain selects entry 16 in the highest-addressed wave;
    # digit 15 in the wave before it, which holds Miller values and takes the generic chain
    assert F.index_of(K_CHUNK - 1) == F.TOP_BOOTH[0] and set(F.TOP_BOOTH) <= set(F.wave_indices(-1))
    assert set(F.TOP_NIBBLE) <= set(F.wave_indices(-2)) and set(F.MILLER) & set(F.wave_indices(-2))
    for w in (-1, -2):                                     # 0, 1 and r - 1 in both
        assert {0, 1, O.R - 1} <= {k[r] for r in F.wave_indices(w)}
    # the stored powers agree with a second route: x^0 = 1, x^1 = x, and x^(r-1) * x = 1 on Gt
    assert np.array_equal(b.pow[0], b.gt_one) and np.array_equal(b.pow[1], b.f[1])
    assert np.array_equal(O.binary("orc_fq12_mul", b.pow[2], b.f[2], 48, 48, 48)[0], b.gt_one)
    assert not b.pow[F.ZERO_ROW].any()
    # g2_mul_many: the zero bases and 0, 1, r - 1 are in the block
    assert np.array_equal(b.g2_mul[1], b.q[1]) and not b.g2_mul[0, 16:].any()
    assert all(not b.g2_mul[r, 16:].any() for r in F.G2_ZERO)


def test_staged_seam_blocks(b):
    st = b.g2_dec[1]
    assert b.b65.shape == (F.PERIOD, 65) and (st == 0).sum() == F.PERIOD - 48
    assert {0, O.CURVE_INVALID_ENCODING} < set(st) and len(set(st)) >= 3
    # valid and invalid records in the chunk's last wave and on both sides of the seam
    assert len(set(st[F.wave_indices(-1)])) >= 2 and (st[:64] == 0).any() and (st[:64] != 0).any()
    assert b.sqrt_ok.any() and not b.sqrt_ok.all() and b.sqrt_ok[0] and not b.sq[0].any()
    assert set(b.eq) == {0, 1} and b.eq[::2].all()
    assert b.add.shape == (F.PERIOD, 24) and not b.add[21, 16:].any()      # a + (-a) = zero
    assert np.array_equal(b.add[20], O.unary("orc_g2_double", b.q[20:21], 24)[0][0])               # a + a
    assert set(b.fq2[1]) == {0, O.FIELD_NOT_MEMBER} and b.b64.shape == (F.PERIOD, 64)
