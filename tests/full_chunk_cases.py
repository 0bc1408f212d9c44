"""Shared by tests/test_full_chunk_cases.py and tests/test_gpu_full_chunk.py: inputs for calls of
one full launch set (kChunk = 2^18 elements, kernels.h) and of one element more, and the oracle's
answer for every row.  CPU only, oracle only, every input from one SplitMix64 seed (SEED).

Each case is a block of PERIOD = 251 distinct rows tiled to n rows: row i of the call is row
i % 251 of the block, the oracle computes the 251 rows and the expected output is the tiled
block, so every output row of a 2^18-row call is compared for the cost of 251 oracle rows.  251
is prime: a row read from an address that is off by any power of two -- a 32-bit wrap of a byte
offset, a truncated index -- is another row of the block, never the same one.

Where the rows of the block lie at n = 2^18 (2^18 % 251 = 100; index_of(), wave_indices()): the
chunk's last row is row 99 of the block, its last wave of 32 elements rows 68 .. 99, the wave
before it rows 36 .. 67, and the one-element set that follows a full one is row 100.  The blocks
put their edge rows there (the constants below); tests/test_full_chunk_cases.py asserts the
placement by index arithmetic."""
import functools

import numpy as np

from oracle import oracle as O
from tests.codec_util import be, compress_g2, subgroup_affine

SEED = 0xf011_c4a7_2026
NT = 16
PERIOD = 251
CHUNK = 1 << 18          # kChunk
N, N1 = CHUNK, CHUNK + 1
WAVE = 32                # elements of a 64-lane wave of the two-lane kernels (kPathLanes = 2)

# ---- rows of the period block (all < PERIOD)
AFFINE_PAIR = 3          # both points normalized: z == one
G1_ZERO = (7, 90)        # G1::zero() paired with a point: Gt::one(); the second in the chunk's last wave
G2_ZERO = (11, 97)       # G2::zero()
MILLER = (40, 50, 130, 200)   # Fq12 rows that are Miller values: outside the cyclotomic subgroup
ZERO_ROW = 45            # the all-zero Fq12 row
TOP_BOOTH = (99, 80)     # scalars whose Booth recoding has a digit of magnitude 16 (table entry 16)
TOP_NIBBLE = (67, 40)    # scalars whose unsigned 4-bit recoding has digit 15 (table entry 15)
EDGE_SCALARS = {0: 0, 1: 1, 2: O.R - 1, 68: 0, 69: 1, 70: O.R - 1, 36: 0, 37: 1, 38: O.R - 1}
# tests/test_gpu_codec.py test_gt_pow's runs: ones and alternating bits (carries, +-16 digits)
RUNS = ((1 << 250) - 1, (1 << 253) - 1, int("01" * 126, 2), int("10000" * 50, 2))
RUN_ROWS = (3, 4, 5, 6)


def index_of(row):
    """The row of the period block that row `row` of a tiled array is."""
    return row % PERIOD


def wave_indices(w, n=CHUNK):
    """The block rows of wave w (0 = first; negative from the end) of an n-element launch set."""
    waves = (n + WAVE - 1) // WAVE
    w = w % waves
    return [index_of(r) for r in range(w * WAVE, min((w + 1) * WAVE, n))]


def tile(block, n):
    """`block` (PERIOD rows) repeated to n rows: row i is block[i % PERIOD]."""
    block = np.asarray(block)
    assert block.shape[0] == PERIOD
    k, r = divmod(n, PERIOD)
    return np.ascontiguousarray(np.concatenate([np.tile(block, (k,) + (1,) * (block.ndim - 1)), block[:r]]))


def _bad_rows(got, block, cols=None):
    """(k, PERIOD) and (r,) boolean arrays: which rows of got differ from the tiled block (on
    the block rows `cols`, a boolean mask, when given).  No second full-size array is built: the
    whole periods of got are viewed as (k, PERIOD, w) against block[None]."""
    got, block = np.asarray(got), np.asarray(block)
    n = got.shape[0]
    assert block.shape[0] == PERIOD and got.shape[1:] == block.shape[1:], (got.shape, block.shape)
    k, r = divmod(n, PERIOD)
    g, b = got.reshape(n, -1), block.reshape(PERIOD, -1)
    head = (g[:k * PERIOD].reshape(k, PERIOD, -1) != b[None]).any(axis=2)
    tail = (g[k * PERIOD:] != b[:r]).any(axis=1)
    if cols is not None:
        head &= np.asarray(cols, bool)[None]
        tail &= np.asarray(cols, bool)[:r]
    return head, tail


def first_mismatch(got, block, cols=None):
    """None when every row of got is its row of the tiled block, else (row, row % PERIOD, row - 2^18)
    of the first one that is not."""
    head, tail = _bad_rows(got, block, cols)
    if head.any():
        row = int(np.argmax(head.reshape(-1)))
    elif tail.any():
        row = head.size + int(np.argmax(tail))
    else:
        return None
    return row, index_of(row), row - CHUNK


def count_mismatches(got, block, cols=None):
    head, tail = _bad_rows(got, block, cols)
    return int(head.sum()) + int(tail.sum())


def assert_tiled(got, block, what, cols=None):
    """Every row of got, bit for bit, against the tiled block."""
    bad = first_mismatch(got, block, cols)
    if bad is not None:
        raise AssertionError("%s: %d of %d rows differ; the first is row %d (block row %d, %+d from 2^18)"
                             % (what, count_mismatches(got, block, cols), np.asarray(got).shape[0], *bad))


# ---- recodings of k_gt_pow (kernels_gtpow.hip)
def booth_digits(k):
    """The 51 signed 5-bit digits k_gt_pow reads off e = 2k: window i is bits 5i .. 5i + 5 of e,
    digit (f >> 1) + (f & 1) - 32 * bit 5."""
    e = 2 * k
    out = []
    for i in range(51):
        f = (e >> (5 * i)) & 63
        out.append((f >> 1) + (f & 1) - (32 if f & 32 else 0))
    assert sum(d << (5 * i) for i, d in enumerate(out)) == k
    return out


def nibbles(k):
    return [(k >> (4 * i)) & 15 for i in range(64)]


def _fr(vals):
    return O.canon_to_mont_array(vals, O.FR).reshape(-1, 4)


def _millers(p, q):
    """bn_miller_loop_many's answer: a pair with a zero point gives Fq12::one()."""
    one = np.zeros(48, np.uint64)
    one[:4] = O.canon_to_mont_array([1])
    out = []
    for k in range(p.shape[0]):
        rc, f = O.miller_loop_batch(q[k:k + 1], p[k:k + 1])
        out.append(one if rc else f)
    return np.stack(out)


def _frob(a, pw):
    out = np.zeros_like(a)
    for k in range(a.shape[0]):
        O.lib().orc_fq12_frobenius_map(O._p(a[k]), pw, O._p(out[k]))
    return out


class _Blocks:
    def __init__(self):
        one = O.canon_to_mont_array([1])
        # ---- pairs: random Jacobian (z != one), one affine pair, zero points on either side
        p, q, _, _ = O.random_pairs(PERIOD, seed=SEED, nthreads=NT)
        p[AFFINE_PAIR] = O.g1_normalize(p[AFFINE_PAIR:AFFINE_PAIR + 1])[0]
        q[AFFINE_PAIR] = O.g2_normalize(q[AFFINE_PAIR:AFFINE_PAIR + 1])[0]
        for r in G1_ZERO:
            p[r] = 0
            p[r, 4:8] = one            # G1::zero() = (0, 1, 0)
        for r in G2_ZERO:
            q[r] = 0
            q[r, 8:12] = one           # G2::zero(): y = (1, 0)
        self.p, self.q = p, q
        self.gt_one = np.zeros(48, np.uint64)
        self.gt_one[:4] = one
        self.e = O.pairing_many(p, q, NT)                 # pairing_many's answer
        self.ml = _millers(p, q)                          # miller_loop_many's answer
        # ---- final_exponentiation_many: the Miller values with one zero row
        self.fe_in = self.ml.copy()
        self.fe_in[ZERO_ROW] = 0
        self.fe_out = self.e.copy()
        self.fe_out[ZERO_ROW] = 0
        self.fe_ok = np.ones(PERIOD, np.uint8)
        self.fe_ok[ZERO_ROW] = 0
        # ---- Fq12 rows: pairing outputs, Miller values, one zero row
        f = self.e.copy()
        for r in MILLER:
            f[r] = self.ml[r]
        f[ZERO_ROW] = 0
        self.f = f
        self.f2 = np.ascontiguousarray(np.roll(f, 17, axis=0))    # the second operand of mul
        self.fq12 = {"mul": O.binary("orc_fq12_mul", f, self.f2, 48, 48, 48),
                     "sqr": O.unary("orc_fq12_squared", f, 48)[0],
                     "inv": O.unary("orc_fq12_inverse", f, 48)[0],
                     "cyc_sqr": O.unary("orc_fq12_cyclotomic_squared", f, 48)[0],
                     "exp_by_neg_z": O.unary("orc_fq12_exp_by_neg_z", f, 48)[0],
                     "frob1": _frob(f, 1), "frob2": _frob(f, 2), "frob3": _frob(f, 3)}
        # ---- scalars
        vals, _ = O.random_scalars(PERIOD, seed=SEED + 1, lo=0)
        for r, v in EDGE_SCALARS.items():
            vals[r] = v
        for r, v in zip(RUN_ROWS, RUNS):
            vals[r] = v
        vals[TOP_BOOTH[0]] = 16 << 245                     # window 49 reads f = 100000 -> digit -16 + carry
        vals[TOP_BOOTH[1]] = (15 << 100) | (31 << 49) | 5  # window 10 reads f = 011111 -> digit +16
        vals[TOP_NIBBLE[0]] = (1 << 253) - 1
        vals[TOP_NIBBLE[1]] = (0xf << 248) | 0xf0f0f
        self.k_vals = [int(v) for v in vals]
        self.k = _fr(self.k_vals)
        self.pow = O.gt_pow(f, self.k)
        self.g2_mul = O.g2_mul(q, self.k, NT)
        # ---- the generic staged() seam: one call per buffer shape
        # 65-byte records, an image and a status: valid and invalid records interleaved as
        # tests/test_gpu_codec.py dev_cases interleaves them
        rng = np.random.default_rng(SEED & 0xffffffff)
        mix = np.random.default_rng((SEED >> 8) & 0xffffffff).permutation(PERIOD)
        g2aff, g1aff = subgroup_affine(PERIOD - 48, SEED + 2, NT)
        c2 = compress_g2(g2aff)
        bad = c2[:48].copy()
        bad[:16, 0] = 12                                    # a bad sign byte
        bad[16:32, 1:] = be(O.P * O.P, 64)                  # x >= p^2
        bad[32:, 1:] = np.stack([be(int.from_bytes(rng.bytes(64), "big") % (O.P * O.P), 64) for _ in range(16)])
        self.b65 = np.ascontiguousarray(np.concatenate([c2, bad])[mix])
        self.g2_dec = O.g2_from_compressed(self.b65, NT)
        # fq_sqrt: zero, residues and non-residues (the image is compared where a root exists)
        g = O.SplitMix64(SEED + 3)
        self.sq = O.canon_to_mont_array([0] + [g.below(O.P) for _ in range(PERIOD - 1)]).reshape(-1, 4)
        self.sqrt, self.sqrt_ok = O.fq_sqrt(self.sq)
        # g1_eq (1-byte output): the same point in another scaling, another point, zero points
        self.eq_a = p
        eq_b = np.ascontiguousarray(np.roll(p, 1, axis=0))
        eq_b[::2] = O.g1_normalize(p[::2])
        self.eq_b = eq_b
        self.eq = np.array(O.g1_eq(self.eq_a, self.eq_b), np.uint8)
        # g2_add (two inputs): other points, a doubling, a + (-a), zero operands
        add_b = np.ascontiguousarray(np.roll(q, 5, axis=0))
        add_b[20] = q[20]
        add_b[21] = O.g2_neg(q[21:22])[0]
        self.add_a, self.add_b = q, add_b
        self.add = O.g2_add(self.add_a, self.add_b)
        # fq2_from_slice (64-byte records): the U512 divrem edges, then random values
        v2 = [0, O.P, O.P * O.P - 1, O.P * O.P, O.P * O.P + 1, (1 << 512) - 1]
        v2 += [int.from_bytes(rng.bytes(64), "big") >> 5 for _ in range(PERIOD - len(v2))]
        self.b64 = np.stack([be(v, 64) for v in v2])
        self.fq2 = O.fq2_from_slice(self.b64)


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)


@functools.lru_cache(maxsize=None)
def blocks():
    """The period blocks and the oracle's answers, computed once and read-only."""
    b = _Blocks()
    for v in vars(b).values():
        _freeze(v)
    return b
