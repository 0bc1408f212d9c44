"""What of the fixed-basis G2 MSM (bn_g2_basis_prepare, bn_g2_msm_basis) needs no device: the
table-size arithmetic of the library, the refusal of every new entry point without a context,
and the argument checks of the Python mirror, which raise before the native call (a stub
stands in for the library there)."""
import ctypes
import os

import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritytech-bn_amd", "libbn254mi.so")
HANDLE = 0x6172


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libbn254mi.so not built (run __graft_entry__.build())"
    return _native.load()


def _windows(c):
    return 254 // c + 1


def test_table_bytes(lib):
    tb = lib.bn_g2_basis_table_bytes
    # W(c) entries of 128 bytes and one flag byte per base
    for nb, c in ((1, 16), (1, 2), (3, 11), (4099, 5), (1 << 20, 16)):
        assert tb(nb, c) == nb * (128 * _windows(c) + 1), (nb, c)
    assert tb(1, 16) == 2049 and tb(1 << 20, 16) == (1 << 31) + (1 << 20)   # 2 KiB per base, 2 GiB at 2^20
    for nb in (1, 4099, 1 << 16, 1 << 18, 1 << 20, 1 << 26):            # 0: the default width for that many bases
        widths = [c for c in range(2, 17) if tb(nb, c) == tb(nb, 0)]
        assert len(widths) >= 1 and _native.g2_basis_table_bytes(nb) == tb(nb, 0) > 0, nb
    # the default is the G2 basis form's own table, pinned on both sides of each of its steps
    # (the widths' window counts all differ, so the byte counts tell them apart)
    for nb, c in ((1, 9), (2047, 9), (2048, 11), (32767, 11), (32768, 12), (92681, 12), (92682, 14), (741454, 14),
                  (741455, 15), (1 << 20, 15), (1 << 26, 15)):
        assert tb(nb, 0) == nb * (128 * _windows(c) + 1), (nb, c)
        assert [w for w in range(2, 17) if tb(nb, w) == tb(nb, 0)] == [c], (nb, c)
    last = 0
    for nb in range(1, 40):
        assert tb(nb, 8) > last
        last = tb(nb, 8)
    # refused arguments give 0
    assert tb(0, 8) == 0 and tb(1, 1) == 0 and tb(1, 17) == 0 and tb(1, -3) == 0
    assert tb(1 << 26, 16) > 0 and tb((1 << 26) + 1, 16) == 0               # more than 2^26 bases
    lim = (2 ** 31 - 1) // _windows(2)
    assert tb(lim, 2) == lim * (128 * 128 + 1) and tb(lim + 1, 2) == 0       # nbases * W(c) over 2^31 - 1
    assert tb(1 << 26, 9) > 0 and tb(1 << 26, 8) == 0                       # W(8) = 32: 2^31 entries
    assert tb(2 ** 60, 16) == 0


def test_every_new_entry_point_refuses_a_null_context(lib):
    buf = np.zeros(64, np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    out = ctypes.c_void_p(0x1234)
    fake = ctypes.c_void_p(HANDLE)
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    assert lib.bn_g2_basis_prepare(None, p, 1, 8, ctypes.byref(out)) == INVALID
    assert lib.bn_g2_basis_prepare_dev(None, p, 1, 8, ctypes.byref(out), None) == INVALID
    assert out.value == 0x1234                       # *out untouched
    assert lib.bn_g2_basis_destroy(None, fake) == INVALID
    assert lib.bn_g2_msm_basis(None, fake, p, 1, p) == INVALID
    assert lib.bn_g2_msm_basis_dev(None, fake, p, 1, p, None) == INVALID
    assert lib.bn_g2_msm_basis(None, None, None, 0, None) == INVALID
    assert lib.bn_g2_msm_basis_reserve(None, fake, 1) == INVALID
    assert lib.bn_g2_basis_count(None) == 0 and lib.bn_g2_basis_window(None) == 0
    assert not buf.any()


class _Lib:
    """Stands in for the native library: records the MSM calls it is handed."""

    def __init__(self, nbases):
        self.nbases = nbases
        self.calls = []
        self.destroyed = []

    def bn_g2_basis_prepare(self, h, bases, nbases, c, out):
        assert nbases == self.nbases
        self.window = c
        out._obj.value = HANDLE
        return _native.BN_OK

    def bn_g2_basis_prepare_dev(self, h, d_bases, nbases, c, out, stream):
        assert nbases == self.nbases
        self.window = c
        self.dev = (d_bases, stream)
        out._obj.value = HANDLE
        return _native.BN_OK

    def bn_g2_basis_count(self, handle):
        return self.nbases

    def bn_g2_basis_window(self, handle):
        return self.window or 12

    def bn_g2_basis_destroy(self, h, handle):
        self.destroyed.append(handle)
        return _native.BN_OK

    def bn_g2_msm_basis(self, h, handle, k, n, out):
        s = np.ctypeslib.as_array(ctypes.cast(k, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 4)).copy()
        self.calls.append({"handle": handle, "k": s, "n": n})
        return _native.BN_OK


def _stub_ctx(nbases):
    c = _native.Context.__new__(_native.Context)
    c._h = ctypes.c_void_p(1)
    c._L = _Lib(nbases)
    c._owner = c      # close() then leaves the stub's fake context handle alone
    return c


def test_scalars_reach_the_library_as_one_prefix():
    c = _stub_ctx(5)
    basis = bn.G2Basis([bn.G2.one()] * 5, window=7, ctx=c)
    assert len(basis) == 5 and basis.count == 5 and basis.window == 7 and not basis.closed
    ks = [bn.Fr.from_int(10 + j) for j in range(3)]
    out = bn.g2_msm_basis(basis, ks)                   # a proper prefix
    assert isinstance(out, bn.G2)
    (call,) = c._L.calls
    want = np.stack([x.img for x in ks])
    assert call["handle"] == HANDLE and call["n"] == 3 and np.array_equal(call["k"], want)
    bn.g2_msm_basis(basis, want)                       # the image array form: the same scalars
    assert np.array_equal(c._L.calls[1]["k"], want)
    assert c.g2_msm_basis(HANDLE, np.zeros((5, 4), np.uint64)).shape == (24,)
    assert np.array_equal(bn.g2_msm_basis(basis, []).img, bn.G2.zero().img) and len(c._L.calls) == 3   # no scalars: no call
    basis.close()
    basis.close()
    assert basis.closed and c._L.destroyed == [HANDLE]
    # the default width is the engine's; a device address takes a count
    with bn.G2Basis([bn.G2.one()] * 5, ctx=c) as b:
        assert b.window == 12
    with bn.G2Basis(0xabc000, window=9, ctx=c, count=5, stream=77) as b:
        assert len(b) == 5 and b.window == 9 and c._L.dev == (0xabc000, 77)


def test_argument_errors_are_raised_before_any_native_call():
    c = _stub_ctx(3)
    basis = bn.G2Basis([bn.G2.one()] * 3, ctx=c)
    one = bn.Fr.from_int(1)
    with pytest.raises(ValueError):
        bn.g2_msm_basis(basis, [one] * 4)                                # more scalars than bases
    with pytest.raises(ValueError):
        c.g2_msm_basis(HANDLE, np.zeros((4, 4), np.uint64))
    with pytest.raises(ValueError):
        c.g2_msm_basis(HANDLE, np.zeros((2, 3), np.uint64))              # not Fr images
    with pytest.raises(ValueError):
        bn.G2Basis([], ctx=c)
    with pytest.raises(ValueError):
        bn.G2Basis([bn.G2.one()], window=17, ctx=c)
    with pytest.raises(ValueError):
        bn.G2Basis([bn.G2.one()], window=1, ctx=c)
    with pytest.raises(ValueError):
        bn.G2Basis(0xabc000, ctx=c)                                      # a device address without a count
    with pytest.raises(ValueError):
        bn.G2Basis([bn.G2.one()] * 3, ctx=c, count=2)
    basis.close()
    with pytest.raises(ValueError):
        bn.g2_msm_basis(basis, [one])
    assert c._L.calls == []


def test_native_mirror_lists_the_new_entry_points():
    for name in ("bn_g2_basis_table_bytes", "bn_g2_basis_prepare", "bn_g2_basis_prepare_dev", "bn_g2_basis_count",
                 "bn_g2_basis_window", "bn_g2_basis_destroy", "bn_g2_msm_basis", "bn_g2_msm_basis_dev",
                 "bn_g2_msm_basis_reserve"):
        assert name in _native.EXPORTS
    for m in ("g2_basis_prepare", "g2_basis_prepare_dev", "g2_basis_count", "g2_basis_window", "g2_basis_destroy",
              "g2_msm_basis", "g2_msm_basis_dev", "g2_msm_basis_reserve"):
        assert callable(getattr(_native.Context, m))
