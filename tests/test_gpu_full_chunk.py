"""Parity at one full launch set and across its seam: every batched entry point that cuts its work
into sets of kChunk = 2^18 elements, at N = 2^18 and N1 = 2^18 + 1, every output row and status
byte bit for bit against the oracle.  Runs on the GPU box: python -m pytest tests -m gpu.

At 2^18 elements the context's workspace (8.6 GB) is addressed where no smaller call reaches: the
32 Fq12 slots of 432 B x n start at t * 432 * n bytes, from slot 19 up at or beyond 2^31 (slot 31
at 3.5e9); the line coefficients (18,792 B per pairing) fill 4.9 GB, past 2^32; k_gt_pow's window
table ends at 1.92e9 of the 2^31 - 1 bytes its 32-bit offsets and buffer descriptor allow.  One row
more makes the chunk loop run a second time: `off * elem` host arithmetic, the stage and workspace
reused for the next set, a one-element set on the latency path right behind a full set on the
throughput path.  tests/test_full_chunk_cases.py states these offsets over the engine's constants.

What makes this cheap is the data (tests/full_chunk_cases.py): 251 distinct rows tiled to n, so the
oracle computes 251 rows and every row of the call is compared; a row fetched from an address off
by a power of two is a different row of the block.

Not covered here: bn_g2_precompute_many past 2^18 (4.4 GB to the host per call) -- the kernels it
runs (k_prepare over the full coefficient region) run in the three-launch form below, but the
`out + off * BN_NUM_COEFFS * 3` of its second set (capi.hip bn_g2_precompute_many) stays untested;
the multi-device forms; the MSM and product families, whose own chunk setters are tested in their
files."""
import numpy as np
import pytest

from tests import full_chunk_cases as F

pytestmark = pytest.mark.gpu
N, N1 = F.N, F.N1


@pytest.fixture(scope="module")
def b():
    return F.blocks()


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiled(b):
    """tiled(name): block `name` tiled to N1 rows, built once, read-only."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = F.tile(getattr(b, name), N1)
            cache[name].setflags(write=False)
        return cache[name]
    return get


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _words(a):
    """the uint64 rows of `a` on the device (int64 storage), as tests/test_gpu_codec.py _words"""
    torch, dev = _torch_dev()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1).copy()).to(dev)


@pytest.fixture(scope="module")
def dev_pairs(tiled):
    """the N1 tiled pairs on the device, shared by the device-form tests"""
    return _words(tiled("p")), _words(tiled("q"))


def _run_dev(call, n, width):
    """call(d_out, stream) on a caller stream -> (n, width) uint64 rows"""
    torch, dev = _torch_dev()
    out = torch.full((n * width,), 0x5a5a, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    call(out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy().view(np.uint64).reshape(n, width)


def _check_gt_one_rows(got, b, what):
    """the zero images' rows are Fq12::one(), at every repetition"""
    for r in F.G1_ZERO + F.G2_ZERO:
        assert (got[r::F.PERIOD] == b.gt_one[None]).all(), "%s: block row %d is not Gt::one() everywhere" % (what, r)


# ---------------------------------------------------------------- pairing
def test_pairing_many_dev_full_set_and_one(ctx, b, dev_pairs):
    """pairing_many_dev at N1 on a caller stream: 2^18 pairs in one k_pairing_full launch (the
    step machine's slots up to 3.6e9 bytes), the last pair on the latency path -- exactly two
    launch sets by bn_get_phase_times."""
    P, Q = dev_pairs
    ctx.set_phase_timing(True)
    try:
        ctx.phase_times()       # (nothing measured before this call)
        got = _run_dev(lambda o, s: ctx.pairing_many_dev(P.data_ptr(), Q.data_ptr(), N1, o, s), N1, 48)
        _, sets = ctx.phase_times()
    finally:
        ctx.set_phase_timing(False)
    ctx.dev_status()
    assert sets == 2
    F.assert_tiled(got, b.e, "pairing_many_dev")
    _check_gt_one_rows(got, b, "pairing_many_dev")


@pytest.mark.parametrize("form", [0, 1, 2])
def test_pairing_many_dev_three_launch_forms(b, dev_pairs, form, monkeypatch):
    """The same call at N under BN254MI_MILLER_FORM: 0 = k_prepare (writes the 4.9 GB coefficient
    region) + k_miller, 1 = k_pairing_fused, 2 = k_prepare + k_miller_seg, each followed by
    k_fq12_vm and k_fe_out (which reads its result slot above 2^31)."""
    from substrate_bn import Context
    monkeypatch.setenv("BN254MI_MILLER_FORM", str(form))
    c = Context(0)
    try:
        P, Q = dev_pairs
        got = _run_dev(lambda o, s: c.pairing_many_dev(P.data_ptr(), Q.data_ptr(), N, o, s), N, 48)
        c.dev_status()
    finally:
        c.close()
    F.assert_tiled(got, b.e, "pairing_many_dev form %d" % form)
    _check_gt_one_rows(got, b, "pairing_many_dev form %d" % form)


def test_pairing_many_host_pageable(b, tiled, monkeypatch):
    """pairing_many at N1 under BN254MI_HOST_PIPELINE=0: the pageable path, whose chunk loop gives
    pairing_many_dev_impl a full set and then one pair."""
    from substrate_bn import Context
    monkeypatch.setenv("BN254MI_HOST_PIPELINE", "0")
    c = Context(0)
    try:
        got = c.pairing_many(tiled("p"), tiled("q"))
    finally:
        c.close()
    F.assert_tiled(got, b.e, "pairing_many (pageable)")
    _check_gt_one_rows(got, b, "pairing_many (pageable)")


def test_pairing_many_host_pipeline(ctx, b, tiled):
    """pairing_many at N1 on the default context: pipelined pieces of 2^17, 2^17 and 1."""
    got = ctx.pairing_many(tiled("p"), tiled("q"))
    F.assert_tiled(got, b.e, "pairing_many (pipeline)")
    _check_gt_one_rows(got, b, "pairing_many (pipeline)")


def test_miller_loop_many(ctx, b, tiled):
    """Host form at N1: k_prepare over the full coefficient region, k_miller, k_gt_store."""
    got = ctx.miller_loop_many(tiled("p"), tiled("q"))
    F.assert_tiled(got, b.ml, "miller_loop_many")
    _check_gt_one_rows(got, b, "miller_loop_many")


def test_final_exponentiation_many(ctx, b, tiled):
    """Host form at N1: k_gt_load, the step machine, k_fe_out with the ok bytes.  The zero row
    gives ok = 0 and a zero image at every repetition, every other row ok = 1."""
    got, ok = ctx.final_exponentiation_many(tiled("fe_in"))
    F.assert_tiled(ok, b.fe_ok, "final_exponentiation_many ok")
    F.assert_tiled(got, b.fe_out, "final_exponentiation_many")
    zero = ok[F.ZERO_ROW::F.PERIOD]
    assert zero.size == N1 // F.PERIOD + 1 and not zero.any() and not got[F.ZERO_ROW::F.PERIOD].any()
    assert int(ok.sum()) == N1 - zero.size and set(np.unique(ok)) == {0, 1}


# ---------------------------------------------------------------- Fq12 operations
UNIT_OPS = [(0, op) for op in ("mul", "sqr", "inv", "cyc_sqr", "exp_by_neg_z", "frob1", "frob2", "frob3")]
UNIT_OPS += [(1, op) for op in ("mul", "sqr", "cyc_sqr", "inv")]


@pytest.mark.parametrize("unit,op", UNIT_OPS)
def test_fq12_op_many(ctx, b, tiled, unit, op):
    """At N1: operands loaded into slots 1 and 2, the result read from slot 3 (k_gt_load,
    k_fq12_vm or -- unit 1 -- k_fq12_vm_pairing, k_gt_store); exp_by_neg_z's chain uses more."""
    ctx.set_fq12_op_unit(unit)
    try:
        got = ctx.fq12_op_many(op, tiled("f"), tiled("f2") if op == "mul" else None)
    finally:
        ctx.set_fq12_op_unit(0)
    F.assert_tiled(got, b.fq12[op], "fq12_op_many %s unit %d" % (op, unit))


# ---------------------------------------------------------------- Gt::pow
def test_gt_pow_many_host(ctx, b, tiled):
    """gt_pow_many (staged) at N1: the window table's 17 entries up to 1.92e9 bytes; the chunk's
    last wave runs the signed chain and selects entry 16, the wave before it the generic chain
    and entry 15 (tests/test_full_chunk_cases.py test_scalar_block)."""
    got = ctx.gt_pow_many(tiled("f"), tiled("k"))
    F.assert_tiled(got, b.pow, "gt_pow_many")


def test_gt_pow_many_dev(ctx, b, tiled):
    A, K = _words(tiled("f")), _words(tiled("k"))
    got = _run_dev(lambda o, s: ctx.gt_pow_many_dev(A.data_ptr(), K.data_ptr(), N1, o, s), N1, 48)
    F.assert_tiled(got, b.pow, "gt_pow_many_dev")


# ---------------------------------------------------------------- G2 * Fr
def test_g2_mul_many(ctx, b, tiled):
    """At N1, raw Jacobian images: zero bases and the scalars 0, 1 and r - 1 in the block."""
    got = ctx.g2_mul_many(tiled("q"), tiled("k"))
    F.assert_tiled(got, b.g2_mul, "g2_mul_many")


# ---------------------------------------------------------------- the generic staged() seam
# One call per buffer shape at N1: a full set, then one element from `off * elem` bytes on.
def test_staged_g2_from_compressed(ctx, b, tiled):
    """65-byte records, an image and a status output"""
    got, st = ctx.g2_from_compressed_many(tiled("b65"))
    F.assert_tiled(st, b.g2_dec[1], "g2_from_compressed_many status")
    F.assert_tiled(got, b.g2_dec[0], "g2_from_compressed_many")


def test_staged_fq_sqrt(ctx, b, tiled):
    got, ok = ctx.fq_sqrt_many(tiled("sq"))
    F.assert_tiled(ok.astype(bool), b.sqrt_ok, "fq_sqrt_many ok")
    F.assert_tiled(got, b.sqrt, "fq_sqrt_many", cols=b.sqrt_ok)     # the root where there is one


def test_staged_g1_eq(ctx, b, tiled):
    """a 1-byte output"""
    got = ctx.group_op_many("g1", "eq", tiled("eq_a"), tiled("eq_b"))
    F.assert_tiled(got, b.eq, "g1_eq_many")


def test_staged_g2_add(ctx, b, tiled):
    """two inputs"""
    got = ctx.group_op_many("g2", "add", tiled("add_a"), tiled("add_b"))
    F.assert_tiled(got, b.add, "g2_add_many")


def test_staged_fq2_from_slice(ctx, b, tiled):
    got, st = ctx.fq2_from_slice_many(tiled("b64"))
    F.assert_tiled(st, b.fq2[1], "fq2_from_slice_many status")
    F.assert_tiled(got, b.fq2[0], "fq2_from_slice_many")
