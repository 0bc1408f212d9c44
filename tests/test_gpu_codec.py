"""GPU parity of SURVEY §8(f) rows 1-4 through the C ABI: encodings, square
roots, AffineG::new validation (incl. the G2 order check), decompression and
Gt::pow, bit-exact (images and per-element status) against the oracle, plus the
reference's known answers.  Runs on the GPU box: python -m pytest tests -m gpu."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.codec_util import be, canon, compress_g1, compress_g2, random_twist_points, subgroup_affine

pytestmark = pytest.mark.gpu
NT = 16
P, R = O.P, O.R


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


def test_field_encodings(ctx):
    rng = np.random.default_rng(5)
    vals = [0, 1, P - 1, P, P + 1, (1 << 256) - 1] + [int.from_bytes(rng.bytes(32), "big") for _ in range(2000)]
    vals += [int.from_bytes(rng.bytes(32), "big") % P for _ in range(2000)]
    b = np.stack([be(v) for v in vals])
    out, st = ctx.fq_from_slice_many(b)
    ref, rst = O.fq_from_slice(b)
    assert np.array_equal(st, rst) and np.array_equal(out, ref)
    ok = st == 0
    assert np.array_equal(ctx.fq_to_big_endian_many(out[ok]), O.fq_to_big_endian(ref[ok]))
    assert np.array_equal(ctx.fr_from_slice_many(b), O.fr_from_slice(b))
    fr = O.fr_from_slice(b)
    assert np.array_equal(ctx.fr_to_big_endian_many(fr), O.fr_to_big_endian(fr))
    # Fq2 / U512 divrem, including the reference's own divrem cases
    v2 = [0, P, P * P - 1, P * P, P * P + 1, (1 << 512) - 1]
    v2 += [int.from_bytes(rng.bytes(64), "big") >> 5 for _ in range(2000)]
    b2 = np.stack([be(v, 64) for v in v2])
    out2, st2 = ctx.fq2_from_slice_many(b2)
    ref2, rst2 = O.fq2_from_slice(b2)
    assert np.array_equal(st2, rst2) and np.array_equal(out2, ref2)


def test_divrem_kats(ctx, kats):
    for c in kats["testing_divrem"]["cases"]:
        out, st = ctx.fq2_from_slice_many(be(int(c["a"]), 64))
        if c["q"] is None:
            assert st[0] == O.FIELD_NOT_MEMBER
        else:
            assert st[0] == 0 and canon(out[0]) == [int(c["r"]), int(c["q"])]


def test_sqrt(ctx, kats):
    k = kats["sqrt_fq"]
    out, ok = ctx.fq_sqrt_many(O.canon_to_mont_array([int(k["square"])]))
    assert ok[0] and canon(out[0]) == [int(k["root"])]
    k = kats["sqrt_fq2"]
    out, ok = ctx.fq2_sqrt_many(O.canon_to_mont_array([int(x) for x in k["square"]]))
    assert ok[0] and canon(out[0]) == [int(x) for x in k["root"]]
    out, ok = ctx.fq2_sqrt_many(O.canon_to_mont_array([P - 1, 0]))
    assert ok[0] and canon(out[0]) == [0, 1]
    _, ok = ctx.fq2_sqrt_many(O.canon_to_mont_array([int(x) for x in k["no_root"]]))
    assert not ok[0]
    g = O.SplitMix64(9)
    a = O.canon_to_mont_array([0] + [g.below(P) for _ in range(1023)]).reshape(-1, 4)
    out, ok = ctx.fq_sqrt_many(a)
    ref, rok = O.fq_sqrt(a)
    assert np.array_equal(ok.astype(bool), rok) and np.array_equal(out[rok], ref[rok])
    a2 = a.reshape(-1, 8)
    out, ok = ctx.fq2_sqrt_many(a2)
    ref, rok = O.fq2_sqrt(a2)
    assert np.array_equal(ok.astype(bool), rok) and np.array_equal(out[rok], ref[rok])


def test_affine_new(ctx):
    g2aff, g1aff = subgroup_affine(64, 31, NT)
    tx, ty = random_twist_points(16, 32)
    ty_bad = ty.copy()
    ty_bad[:, 0] ^= 2
    x = np.concatenate([g2aff[:, :8], tx, tx])
    y = np.concatenate([g2aff[:, 8:], ty, ty_bad])
    out, st = ctx.g2_affine_new_many(x, y)
    ref, rst = O.g2_affine_new(x, y, NT)
    assert list(rst[:64]) == [0] * 64 and list(rst[64:80]) == [7] * 16 and list(rst[80:]) == [6] * 16
    assert np.array_equal(st, rst) and np.array_equal(out, ref)
    out, st = ctx.g1_affine_new_many(g1aff[:, :4], g1aff[:, 4:])
    ref, rst = O.g1_affine_new(g1aff[:, :4], g1aff[:, 4:])
    assert list(st) == [0] * 64 and np.array_equal(out, ref)
    _, st = ctx.g1_affine_new_many(g1aff[:, 4:], g1aff[:, :4])
    assert list(st) == [O.GROUP_NOT_ON_CURVE] * 64


def test_decompression_kats(ctx, kats):
    k = kats["g1_from_compressed"]
    out, st = ctx.g1_from_compressed_many(np.frombuffer(bytes.fromhex(k["bytes"]), np.uint8))
    assert st[0] == 0 and canon(out[0]) == [int(k["x"]), int(k["y"]), 1]
    k = kats["g2_from_compressed"]
    recs = np.stack([np.frombuffer(bytes.fromhex(k[n]), np.uint8)
                     for n in ("bytes_0a", "bytes_0b_negated", "bytes_0c_invalid")])
    out, st = ctx.g2_from_compressed_many(recs)
    assert list(st) == [0, 0, O.CURVE_INVALID_ENCODING]
    assert canon(out[0]) == [int(v) for v in k["x"] + k["y"]] + [1, 0]
    ref, rst = O.g2_from_compressed(recs)
    assert np.array_equal(out, ref) and np.array_equal(st, rst)


def test_decompression_random_and_invalid(ctx):
    g2aff, g1aff = subgroup_affine(512, 41, NT)
    c1 = compress_g1(g1aff)
    c2 = compress_g2(g2aff)
    # invalid variants: bad sign byte, x >= p (G1) / x >= p^2 (G2), random x (no root or not in the subgroup)
    rng = np.random.default_rng(42)
    bad1 = c1[:64].copy()
    bad1[:16, 0] = 4
    bad1[16:32, 1:] = be(P)
    bad1[32:, 1:] = np.stack([be(int.from_bytes(rng.bytes(32), "big") % P) for _ in range(32)])
    bad2 = c2[:64].copy()
    bad2[:16, 0] = 12
    bad2[16:32, 1:] = be(P * P, 64)
    bad2[32:, 1:] = np.stack([be(int.from_bytes(rng.bytes(64), "big") % (P * P), 64) for _ in range(32)])
    a1 = np.concatenate([c1, bad1])
    a2 = np.concatenate([c2, bad2])
    out, st = ctx.g1_from_compressed_many(a1)
    ref, rst = O.g1_from_compressed(a1, NT)
    assert list(rst[:512]) == [0] * 512
    assert np.array_equal(st, rst) and np.array_equal(out, ref)
    assert np.array_equal(out[:512, :8], g1aff)
    out, st = ctx.g2_from_compressed_many(a2)
    ref, rst = O.g2_from_compressed(a2, NT)
    assert list(rst[:512]) == [0] * 512 and set(rst[576 - 32:]) <= {O.CURVE_NOT_MEMBER}
    assert np.array_equal(st, rst) and np.array_equal(out, ref)
    assert np.array_equal(out[:512, :16], g2aff)


def test_gt_pow(ctx):
    p, q, _, _ = O.random_pairs(64, seed=51, nthreads=NT)
    g = O.pairing_many(p, q, NT)
    # non-cyclotomic inputs: Miller values (a Gt may hold a miller_loop_batch output)
    ml = np.stack([O.miller_loop_batch(q[k:k + 1], p[k:k + 1])[1] for k in range(8)])
    a = np.concatenate([g, ml])
    vals, k = O.random_scalars(a.shape[0], 52, lo=0)
    k[0] = O.canon_to_mont_array([0], O.FR)
    k[1] = O.canon_to_mont_array([1], O.FR)
    k[2] = O.canon_to_mont_array([R - 1], O.FR)
    # runs of ones and alternating bits (the signed 5-bit windows' carries and +-16 digits)
    k[3:7] = O.canon_to_mont_array([(1 << 250) - 1, (1 << 253) - 1, int("01" * 126, 2), int("10000" * 50, 2)],
                                   O.FR).reshape(4, 4)
    out = ctx.gt_pow_many(a, k)
    assert np.array_equal(out, O.gt_pow(a, k))
    # waves holding only pairing outputs take the cyclotomic squarings, the rest the
    # generic ones: a Miller value and a zero element inside an otherwise cyclotomic wave
    b = np.concatenate([g[:10], ml[:1], g[10:40], np.zeros((1, 48), np.uint64), g[40:], ml[1:]])
    kb = np.concatenate([k, k[:1]])
    out = ctx.gt_pow_many(b, kb)
    assert np.array_equal(out, O.gt_pow(b, kb))


# ---------------------------------------------------------------- the device-pointer forms
DEV_SIZES = [1, 63, 64, 65, 129]
NDEV = 129
INVALID_ARGUMENT = 1


@pytest.fixture(scope="module")
def dev_cases():
    """129 inputs of each _dev call, built as the host-form tests above build theirs -- valid
    and invalid records interleaved by a fixed permutation -- and the oracle's images and
    status bytes, computed once; every size takes a prefix."""
    rng = np.random.default_rng(43)
    mix = np.random.default_rng(44).permutation(NDEV)
    g2aff, g1aff = subgroup_affine(97, 61, NT)
    # compressed records: 97 valid, then a bad sign byte, x >= p (p^2 for G2) and a random x
    c1, c2 = compress_g1(g1aff), compress_g2(g2aff)
    bad1, bad2 = c1[:32].copy(), c2[:32].copy()
    bad1[:8, 0] = 4
    bad1[8:16, 1:] = be(P)
    bad1[16:, 1:] = np.stack([be(int.from_bytes(rng.bytes(32), "big") % P) for _ in range(16)])
    bad2[:8, 0] = 12
    bad2[8:16, 1:] = be(P * P, 64)
    bad2[16:, 1:] = np.stack([be(int.from_bytes(rng.bytes(64), "big") % (P * P), 64) for _ in range(16)])
    b33 = np.ascontiguousarray(np.concatenate([c1, bad1])[mix])
    b65 = np.ascontiguousarray(np.concatenate([c2, bad2])[mix])
    # AffineG2::new: 97 subgroup points, 16 twist points outside it, 16 points off the curve
    tx, ty = random_twist_points(16, 62)
    ty_bad = ty.copy()
    ty_bad[:, 0] ^= 2
    x = np.ascontiguousarray(np.concatenate([g2aff[:, :8], tx, tx])[mix])
    y = np.ascontiguousarray(np.concatenate([g2aff[:, 8:], ty, ty_bad])[mix])
    # Gt::pow: test_gt_pow's mixed rows -- pairing outputs, a Miller value and a zero element
    # inside the first wave, more Miller values behind -- and its planted scalars
    p, q, _, _ = O.random_pairs(64, seed=51, nthreads=NT)
    g = O.pairing_many(p, q, NT)
    ml = np.stack([O.miller_loop_batch(q[k:k + 1], p[k:k + 1])[1] for k in range(8)])
    b = np.concatenate([g[:10], ml[:1], g[10:40], np.zeros((1, 48), np.uint64), g[40:], ml[1:]])
    a = np.ascontiguousarray(np.concatenate([b, b[:NDEV - b.shape[0]]]))
    _, k = O.random_scalars(NDEV, 63, lo=0)
    k[:3] = O.canon_to_mont_array([0, 1, R - 1], O.FR).reshape(3, 4)
    k[3:7] = O.canon_to_mont_array([(1 << 250) - 1, (1 << 253) - 1, int("01" * 126, 2), int("10000" * 50, 2)],
                                   O.FR).reshape(4, 4)
    d = {"b33": b33, "g1": O.g1_from_compressed(b33, NT), "b65": b65, "g2": O.g2_from_compressed(b65, NT),
         "x": x, "y": y, "aff": O.g2_affine_new(x, y, NT), "a": a, "k": k, "pow": O.gt_pow(a, k)}
    # valid and invalid records in every prefix of 63 and more
    for key in ("g1", "g2"):
        st = d[key][1]
        assert (st[:63] == 0).any() and len(set(st[:63])) >= 3, (key, sorted(set(st)))
    assert set(d["aff"][1][:63]) == {0, 6, 7}  # ok, NotOnCurve, NotInSubgroup
    return d


def _torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def _words(a):
    """the uint64 rows of `a` on the device (int64 storage)"""
    torch, dev = _torch_dev()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1).copy()).to(dev)


def _bytes_at(a, shift):
    """the bytes of `a` on the device, starting `shift` bytes into a fresh allocation"""
    torch, dev = _torch_dev()
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    raw = torch.zeros(a.size + 8, dtype=torch.uint8, device=dev)
    view = raw[shift:shift + a.size]
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % 8 == shift % 8
    return view, raw


def _run_dev(ctx, call, n, width, st_shift=0):
    """call(d_out, d_status, stream) on a caller stream -> ((n, width) images, n status bytes)"""
    torch, dev = _torch_dev()
    out = torch.full((n * width,), 0x5a5a, dtype=torch.int64, device=dev)
    sraw = torch.full((n + 8,), 0x5a, dtype=torch.uint8, device=dev)
    st = sraw[st_shift:st_shift + n]
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    call(out.data_ptr(), st.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(dev)
    guard = sraw.cpu().numpy()
    assert (guard[:st_shift] == 0x5a).all() and (guard[st_shift + n:] == 0x5a).all(), "status bytes written outside [0, n)"
    return out.cpu().numpy().view(np.uint64).reshape(n, width), guard[st_shift:st_shift + n]


@pytest.mark.parametrize("shift,st_shift", [(0, 0), (1, 3)])
@pytest.mark.parametrize("n", DEV_SIZES)
def test_g1_from_compressed_dev(ctx, dev_cases, n, shift, st_shift):
    """33-byte records carry no alignment: also with the records from an odd device address
    and the status bytes from another."""
    ref, rst = dev_cases["g1"]
    B, _raw = _bytes_at(dev_cases["b33"][:n], shift)
    out, st = _run_dev(ctx, lambda o, t, s: ctx.g1_from_compressed_many_dev(B.data_ptr(), n, o, t, s), n, 12, st_shift)
    assert np.array_equal(st, rst[:n]) and np.array_equal(out, ref[:n])


@pytest.mark.parametrize("shift,st_shift", [(0, 0), (1, 3)])
@pytest.mark.parametrize("n", DEV_SIZES)
def test_g2_from_compressed_dev(ctx, dev_cases, n, shift, st_shift):
    ref, rst = dev_cases["g2"]
    B, _raw = _bytes_at(dev_cases["b65"][:n], shift)
    out, st = _run_dev(ctx, lambda o, t, s: ctx.g2_from_compressed_many_dev(B.data_ptr(), n, o, t, s), n, 24, st_shift)
    assert np.array_equal(st, rst[:n]) and np.array_equal(out, ref[:n])


@pytest.mark.parametrize("n", DEV_SIZES)
def test_g2_affine_new_dev(ctx, dev_cases, n):
    ref, rst = dev_cases["aff"]
    X, Y = _words(dev_cases["x"][:n]), _words(dev_cases["y"][:n])
    out, st = _run_dev(ctx, lambda o, t, s: ctx.g2_affine_new_many_dev(X.data_ptr(), Y.data_ptr(), n, o, t, s), n, 24)
    assert np.array_equal(st, rst[:n]) and np.array_equal(out, ref[:n])


@pytest.mark.parametrize("n", DEV_SIZES)
def test_gt_pow_dev(ctx, dev_cases, n):
    A, K = _words(dev_cases["a"][:n]), _words(dev_cases["k"][:n])
    out, _ = _run_dev(ctx, lambda o, t, s: ctx.gt_pow_many_dev(A.data_ptr(), K.data_ptr(), n, o, s), n, 48)
    assert np.array_equal(out, dev_cases["pow"][:n])


def test_dev_forms_null_arguments(ctx, dev_cases):
    """n == 0 with NULL pointers is BN_OK and touches nothing; a NULL buffer with n > 0 is
    refused (each buffer in turn, the others real)."""
    torch, dev = _torch_dev()
    L, h = ctx._L, ctx.handle
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    d = buf.data_ptr()
    assert L.bn_g1_from_compressed_many_dev(h, None, 0, None, None, None) == 0
    assert L.bn_g2_from_compressed_many_dev(h, None, 0, None, None, None) == 0
    assert L.bn_g2_affine_new_many_dev(h, None, None, 0, None, None, None) == 0
    assert L.bn_gt_pow_many_dev(h, None, None, 0, None, None) == 0
    for fn in (L.bn_g1_from_compressed_many_dev, L.bn_g2_from_compressed_many_dev):
        for args in ((None, 1, d, d), (d, 1, None, d), (d, 1, d, None)):
            assert fn(h, *args, None) == INVALID_ARGUMENT
    for args in ((None, d, 1, d, d), (d, None, 1, d, d), (d, d, 1, None, d), (d, d, 1, d, None)):
        assert L.bn_g2_affine_new_many_dev(h, *args, None) == INVALID_ARGUMENT
    for args in ((None, d, 1, d), (d, None, 1, d), (d, d, 1, None)):
        assert L.bn_gt_pow_many_dev(h, *args, None) == INVALID_ARGUMENT
    torch.cuda.synchronize(dev)
    assert not buf.cpu().numpy().any()
    # the context is still good
    n = 5
    A, K = _words(dev_cases["a"][:n]), _words(dev_cases["k"][:n])
    out, _ = _run_dev(ctx, lambda o, t, s: ctx.gt_pow_many_dev(A.data_ptr(), K.data_ptr(), n, o, s), n, 48)
    assert np.array_equal(out, dev_cases["pow"][:n])


def test_rust_api_mirror_codec(kats):
    import substrate_bn as bn
    k = kats["g1_from_compressed"]
    g = bn.G1.from_compressed(bytes.fromhex(k["bytes"]))
    assert g.x().into_int() == int(k["x"]) and g.y().into_int() == int(k["y"])
    with pytest.raises(bn.CurveError):
        bn.G2.from_compressed(bytes.fromhex(kats["g2_from_compressed"]["bytes_0c_invalid"]))
    with pytest.raises(bn.FieldError):
        bn.Fq.from_slice(P.to_bytes(32, "big"))
    assert bn.Fq.from_slice((5).to_bytes(32, "big")).to_big_endian() == (5).to_bytes(32, "big")
    assert bn.Fr.from_slice(R.to_bytes(32, "big")) == bn.Fr.zero()
    tx, ty = random_twist_points(1, 77)
    with pytest.raises(bn.GroupError):
        bn.AffineG2.new(bn.Fq2(tx[0]), bn.Fq2(ty[0]))
    gt = bn.pairing(bn.G1.one(), bn.G2.one())
    assert gt.pow(bn.Fr.from_int(3)) == gt * gt * gt
