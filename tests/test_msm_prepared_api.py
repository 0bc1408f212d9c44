"""What of the prepared-bases MSM (bn_g1_bases_prepare, bn_g1_msm_prepared_many) needs no
device: the table-size arithmetic of the library, the refusal of every new entry point
without a context, and the argument checks of the Python mirror, which raise before the
native call (a stub stands in for the library there)."""
import ctypes
import os

import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritytech-bn_amd", "libbn254mi.so")
HANDLE = 0x6171


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libbn254mi.so not built (run __graft_entry__.build())"
    return _native.load()


def _entries(k, c):
    return k * (254 // c + 1) * (1 << (c - 1))


def test_table_bytes(lib):
    tb = lib.bn_g1_prepared_table_bytes
    for k, c in ((1, 8), (16, 8)):
        got = tb(k, c)
        assert got >= _entries(k, c) * 64            # the entries ...
        assert got - _entries(k, c) * 64 <= 64 * k   # ... plus whatever the zero flags take
    assert tb(1, 8) == 32 * 128 * 64 + 1 and tb(16, 8) == 16 * 32 * 128 * 64 + 16
    assert tb(3, 0) == tb(3, 10) and _native.g1_prepared_table_bytes(3) == tb(3, 10)  # 0: the default width
    last = 0
    for k in range(1, 40):
        assert tb(k, 8) > last
        last = tb(k, 8)
    assert tb(1, 1) == 0 and tb(1, 17) == 0 and tb(0, 8) == 0 and tb(1, -3) == 0
    kmax = (2 ** 31 - 1) // _entries(1, 8)
    assert tb(kmax, 8) == kmax * _entries(1, 8) * 64 + kmax
    assert tb(kmax + 1, 8) == 0                      # an entry count over 2^31 - 1
    assert tb(2 ** 31 // _entries(1, 16), 16) == 0 and tb(2 ** 31 // _entries(1, 16) - 1, 16) > 0
    assert tb(2 ** 60, 8) == 0


def test_every_new_entry_point_refuses_a_null_context(lib):
    buf = np.zeros(64, np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    out = ctypes.c_void_p(0x1234)
    fake = ctypes.c_void_p(HANDLE)
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    assert lib.bn_g1_bases_prepare(None, p, 1, 8, ctypes.byref(out)) == INVALID
    assert lib.bn_g1_bases_prepare_dev(None, p, 1, 8, ctypes.byref(out), None) == INVALID
    assert out.value == 0x1234                       # *out untouched
    assert lib.bn_g1_prepared_destroy(None, fake) == INVALID
    assert lib.bn_g1_msm_prepared_many(None, fake, p, 1, p, 1) == INVALID
    assert lib.bn_g1_msm_prepared_many_dev(None, fake, p, 1, p, 1, None) == INVALID
    assert lib.bn_g1_msm_prepared_many(None, None, None, 0, None, 1) == INVALID
    for lanes in (0, 1, 64, 3):
        assert lib.bn_set_msm_prepared_lanes(None, lanes) == INVALID
    assert lib.bn_g1_prepared_count(None) == 0 and lib.bn_g1_prepared_window(None) == 0


class _Lib:
    """Stands in for the native library: records the MSM calls it is handed."""

    def __init__(self, k):
        self.k = k
        self.calls = []

    def bn_g1_bases_prepare(self, h, bases, k, c, out):
        assert k == self.k
        self.window = c
        out._obj.value = HANDLE
        return _native.BN_OK

    def bn_g1_prepared_count(self, handle):
        return self.k

    def bn_g1_prepared_window(self, handle):
        return self.window or 10

    def bn_g1_prepared_destroy(self, h, handle):
        return _native.BN_OK

    def bn_g1_msm_prepared_many(self, h, handle, k, m, out, out_stride):
        s = np.ctypeslib.as_array(ctypes.cast(k, ctypes.POINTER(ctypes.c_uint64)), shape=(m, self.k, 4)).copy()
        self.calls.append({"handle": handle, "k": s, "m": m, "stride": out_stride})
        return _native.BN_OK


def _prepared(k, window=0):
    c = _native.Context.__new__(_native.Context)
    c._h = ctypes.c_void_p(1)
    c._L = _Lib(k)
    c._owner = c      # close() then leaves the stub's fake context handle alone
    return c, bn.G1Prepared([bn.G1.one()] * k, window=window, ctx=c)


def test_rows_reach_the_library_as_one_row_major_matrix():
    c, prep = _prepared(3, window=5)
    assert len(prep) == 3 and prep.window == 5 and not prep.closed
    rows = [[bn.Fr.from_int(10 * j + b) for b in range(3)] for j in range(4)]
    out = bn.g1_msm_prepared_many(prep, rows)
    assert len(out) == 4 and all(isinstance(g, bn.G1) for g in out)
    (call,) = c._L.calls
    assert call["handle"] == HANDLE and call["m"] == 4 and call["stride"] == 1
    want = np.stack([np.stack([x.img for x in r]) for r in rows])
    assert np.array_equal(call["k"], want)
    bn.g1_msm_prepared_many(prep, want)              # the image array form: the same matrix
    assert np.array_equal(c._L.calls[1]["k"], want)
    assert c.g1_msm_prepared_many(HANDLE, want, out_stride=4).shape == (16, 12)
    assert c._L.calls[2]["stride"] == 4
    assert bn.g1_msm_prepared_many(prep, []) == [] and len(c._L.calls) == 3   # no rows: no call


def test_argument_errors_are_raised_before_any_native_call():
    c, prep = _prepared(3)
    one = bn.Fr.from_int(1)
    with pytest.raises(ValueError):
        bn.g1_msm_prepared_many(prep, [[one, one, one], [one, one]])
    with pytest.raises(ValueError):
        bn.g1_msm_prepared_many(prep, np.zeros((2, 4, 4), np.uint64))
    with pytest.raises(ValueError):
        c.g1_msm_prepared_many(HANDLE, np.zeros((2, 2, 4), np.uint64))    # width 2 for 3 bases
    with pytest.raises(ValueError):
        c.g1_msm_prepared_many(HANDLE, np.zeros((2, 4), np.uint64))      # a bare (m, 4) needs one base
    with pytest.raises(ValueError):
        c.g1_msm_prepared_many(HANDLE, np.zeros((2, 3, 4), np.uint64), out_stride=0)
    with pytest.raises(ValueError):
        c.g1_msm_prepared_many_dev(HANDLE, 0, 2, 0, out_stride=0)
    with pytest.raises(ValueError):
        bn.G1Prepared([], ctx=c)
    with pytest.raises(ValueError):
        bn.G1Prepared([bn.G1.one()], window=17, ctx=c)
    prep.close()
    assert prep.closed
    with pytest.raises(ValueError):
        bn.g1_msm_prepared_many(prep, [[one, one, one]])
    assert c._L.calls == []


def test_native_mirror_lists_the_new_entry_points():
    for name in ("bn_g1_prepared_table_bytes", "bn_g1_bases_prepare", "bn_g1_bases_prepare_dev", "bn_g1_prepared_count",
                 "bn_g1_prepared_window", "bn_g1_prepared_destroy", "bn_g1_msm_prepared_many",
                 "bn_g1_msm_prepared_many_dev", "bn_set_msm_prepared_lanes"):
        assert name in _native.EXPORTS
    for m in ("g1_bases_prepare", "g1_bases_prepare_dev", "g1_prepared_count", "g1_prepared_window",
              "g1_prepared_destroy", "g1_msm_prepared_many", "g1_msm_prepared_many_dev", "set_msm_prepared_lanes"):
        assert callable(getattr(_native.Context, m))
