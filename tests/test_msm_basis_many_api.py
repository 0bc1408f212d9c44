"""What of the batched fixed-basis MSM (bn_g1_msm_basis_many) needs no device: the exports,
the refusal of every new entry point without a context, the argument checks of the Python
mirror, which raise before the native call (a stub stands in for the library there), m == 0,
and the set-size arithmetic of csrc/msm_basis_many.h (through its host build).  The refusals
that need a live context and handle are in tests/test_gpu_msm_basis_many.py."""
import ctypes
import os

import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native
from tests.native import msmbasismanyemul as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritytech-bn_amd", "libbn254mi.so")
HANDLE = 0x6173
NEW = ("bn_g1_msm_basis_many", "bn_g1_msm_basis_many_dev", "bn_g1_msm_basis_many_reserve", "bn_set_msm_basis_many_set")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libbn254mi.so not built (run __graft_entry__.build())"
    return _native.load()


def test_native_mirror_lists_the_new_entry_points(lib):
    for name in NEW:
        assert name in _native.EXPORTS
        assert getattr(lib, name) is not None
    for m in ("g1_msm_basis_many", "g1_msm_basis_many_dev", "g1_msm_basis_many_reserve", "set_msm_basis_many_set"):
        assert callable(getattr(_native.Context, m))
    assert callable(bn.g1_msm_basis_many)


def test_every_new_entry_point_refuses_a_null_context(lib):
    buf = np.zeros(64, np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    fake = ctypes.c_void_p(HANDLE)
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    assert lib.bn_g1_msm_basis_many(None, fake, p, 1, 1, 1, p, 1) == INVALID
    assert lib.bn_g1_msm_basis_many(None, fake, p, 1, 0, 1, p, 1) == INVALID         # also with m == 0
    assert lib.bn_g1_msm_basis_many_dev(None, fake, p, 1, 1, 1, p, 1, None) == INVALID
    assert lib.bn_g1_msm_basis_many(None, None, None, 0, 0, 0, None, 0) == INVALID
    assert lib.bn_g1_msm_basis_many_reserve(None, fake, 1, 1) == INVALID
    assert lib.bn_set_msm_basis_many_set(None, 2) == INVALID
    assert not buf.any()


class _Lib:
    """Stands in for the native library: records the batched calls it is handed."""

    def __init__(self, nbases):
        self.nbases = nbases
        self.calls = []

    def bn_g1_basis_prepare(self, h, bases, nbases, c, out):
        out._obj.value = HANDLE
        return _native.BN_OK

    def bn_g1_basis_count(self, handle):
        return self.nbases

    def bn_g1_basis_window(self, handle):
        return 12

    def bn_g1_basis_destroy(self, h, handle):
        return _native.BN_OK

    def bn_g1_msm_basis_many(self, h, handle, k, k_stride, m, n, out, out_stride):
        s = None
        if k is not None:
            s = np.ctypeslib.as_array(ctypes.cast(k, ctypes.POINTER(ctypes.c_uint64)), shape=(m, k_stride, 4)).copy()
        self.calls.append({"handle": handle, "k": s, "k_stride": k_stride, "m": m, "n": n, "out_stride": out_stride})
        return _native.BN_OK

    def bn_g1_msm_basis_many_dev(self, h, handle, d_k, k_stride, m, n, d_out, out_stride, stream):
        self.calls.append({"dev": (d_k, k_stride, m, n, d_out, out_stride, stream)})
        return _native.BN_OK

    def bn_g1_msm_basis_many_reserve(self, h, handle, m, n):
        self.calls.append({"reserve": (m, n)})
        return _native.BN_OK

    def bn_set_msm_basis_many_set(self, h, vectors):
        self.calls.append({"set": vectors})
        return _native.BN_OK


def _stub_ctx(nbases):
    c = _native.Context.__new__(_native.Context)
    c._h = ctypes.c_void_p(1)
    c._L = _Lib(nbases)
    c._owner = c      # close() then leaves the stub's fake context handle alone
    return c


def test_rows_reach_the_library_with_their_stride():
    c = _stub_ctx(5)
    basis = bn.G1Basis([bn.G1.one()] * 5, ctx=c)
    rows = [[bn.Fr.from_int(10 * j + i + 1) for i in range(3)] for j in range(2)]
    out = bn.g1_msm_basis_many(basis, rows)                       # a proper prefix, two rows
    assert out.shape == (2, 12)
    (call,) = c._L.calls
    want = np.stack([np.stack([x.img for x in r]) for r in rows])
    assert call["handle"] == HANDLE and (call["m"], call["n"], call["k_stride"], call["out_stride"]) == (2, 3, 3, 1)
    assert np.array_equal(call["k"], want)
    assert bn.g1_msm_basis_many(basis, want).shape == (2, 12)     # the image array form: the same scalars
    assert np.array_equal(c._L.calls[1]["k"], want)
    # the mirror: n below the row length (a wider matrix), an output stride
    wide = np.arange(2 * 5 * 4, dtype=np.uint64).reshape(2, 5, 4)
    assert c.g1_msm_basis_many(HANDLE, wide, n=2, out_stride=3).shape == (6, 12)
    last = c._L.calls[2]
    assert (last["m"], last["n"], last["k_stride"], last["out_stride"]) == (2, 2, 5, 3) and np.array_equal(last["k"], wide)
    assert c.g1_msm_basis_many(HANDLE, wide, n=0).shape == (2, 12) and c._L.calls[3]["k"] is None   # n == 0: no scalars read
    # m == 0: no call at all
    assert bn.g1_msm_basis_many(basis, []).shape == (0, 12)
    assert c.g1_msm_basis_many(HANDLE, np.zeros((0, 3, 4), np.uint64)).shape == (0, 12)
    assert len(c._L.calls) == 4
    c.g1_msm_basis_many_dev(HANDLE, 0x1000, 7, 2, 5, 0x2000, out_stride=2, stream=9)
    assert c._L.calls[4] == {"dev": (0x1000, 7, 2, 5, 0x2000, 2, 9)}
    c.g1_msm_basis_many_reserve(HANDLE, 16, 5)
    c.set_msm_basis_many_set(2)
    assert c._L.calls[5:] == [{"reserve": (16, 5)}, {"set": 2}]


def test_argument_errors_are_raised_before_any_native_call():
    c = _stub_ctx(3)
    basis = bn.G1Basis([bn.G1.one()] * 3, ctx=c)
    one = bn.Fr.from_int(1)
    with pytest.raises(ValueError):
        bn.g1_msm_basis_many(basis, [[one] * 4])                         # a row longer than the basis
    with pytest.raises(ValueError):
        bn.g1_msm_basis_many(basis, [[one] * 2, [one] * 3])              # ragged rows
    with pytest.raises(ValueError):
        bn.g1_msm_basis_many(basis, np.zeros((2, 4), np.uint64))         # not rows of Fr images
    with pytest.raises(ValueError):
        c.g1_msm_basis_many(HANDLE, np.zeros((2, 3, 3), np.uint64))
    with pytest.raises(ValueError):
        c.g1_msm_basis_many(HANDLE, np.zeros((2, 4, 4), np.uint64))      # n above the handle's count
    with pytest.raises(ValueError):
        c.g1_msm_basis_many(HANDLE, np.zeros((2, 2, 4), np.uint64), n=3)  # n above the row length
    with pytest.raises(ValueError):
        c.g1_msm_basis_many(HANDLE, np.zeros((2, 2, 4), np.uint64), out_stride=0)
    with pytest.raises(ValueError):
        c.g1_msm_basis_many_dev(HANDLE, 0x1000, 2, 1, 2, 0x2000, out_stride=0)
    with pytest.raises(ValueError):
        c.g1_msm_basis_many_dev(HANDLE, 0x1000, 2, 1, 3, 0x2000)          # k_stride below n
    basis.close()
    with pytest.raises(ValueError):
        bn.g1_msm_basis_many(basis, [[one]])
    assert c._L.calls == []


def _windows(c):
    return 254 // c + 1


def _nkeys(c):
    return _windows(c) << (c - 1)


def test_set_size_arithmetic():
    S = E.set_size
    # the bound on bucket memory: S * nkeys <= 2^23 by default, at most m, at least 1
    for c in (2, 5, 10, 12, 14, 16):
        want = (1 << 23) // _nkeys(c)
        assert S(1 << 26, 1, c) == want, c
        assert S(want + 1, 1, c) == want and S(want, 1, c) == want and S(3, 1, c) == min(3, want)
        assert want * _nkeys(c) <= 1 << 23 < (want + 1) * _nkeys(c)
    assert S(1 << 26, 65, 16) == 16                       # 2^19 keys per vector: the smallest default S
    assert S(1, 1 << 20, 16) == 1 and S(0, 5, 10) == 1    # never 0
    for keys in (1 << 21, 1 << 22):                       # another bound
        assert S(1 << 26, 1, 10, max_keys=keys) == keys // _nkeys(10)
    assert S(1 << 26, 1, 16, max_keys=1) == 1             # a bound below one vector's keys: still 1
    # the entry bound: S * n * W(c) <= 2^31 - 1 whatever else is asked
    lim = 2 ** 31 - 1
    n = 1 << 20
    assert S(1 << 26, n, 2) == lim // (n * 128) == 15     # the bucket bound alone would give 2^22
    assert S(1 << 26, n, 2, forced=16) == 15 and S(1 << 26, n, 2, forced=15) == 15 and S(1 << 26, n, 2, forced=7) == 7
    assert S(1 << 26, lim // 128, 2) == 1 and S(1 << 26, (1 << 26), 9, forced=5) == 1
    for n, c in ((3, 2), (1000, 5), (1 << 18, 14)):
        s = S(1 << 26, n, c, forced=1 << 26)
        assert s * n * _windows(c) <= lim and (s == 1 << 26 or (s + 1) * n * _windows(c) > lim
                                                 or (s + 1) * (4 * _nkeys(c) + 2) > 2 ** 32 - 1), (n, c, s)
    # forcing: takes the place of the bucket bound, still at most m
    assert S(17, 1000, 10, forced=2) == 2 and S(17, 1000, 10, forced=16) == 16 and S(5, 1000, 10, forced=16) == 5
    assert S(1 << 26, 8, 16, forced=64) == 64
    # a vector's block of integer words keeps its 32-bit index
    assert S(1 << 26, 1, 2, forced=1 << 26) * (4 * _nkeys(2) + 2) <= 2 ** 32 - 1
    # the level-0 slots of a set (at most 2 n W(c) per vector, at run cap 1) stay 32-bit with the entries
    n, c = 1 << 16, 2
    s = S(1 << 26, n, c, forced=1 << 20)
    nent = n * 128
    assert s == lim // nent and s * (nent + min(nent // 2, _nkeys(c))) <= 2 ** 32 - 1
