"""What of bn_g1_msm_many needs no device: the refusal of every new entry point without a
context, the argument checks of the Python mirror, which raise before the native call (a
stub stands in for the library there), the empty call, and the entry points listed in
_native."""
import ctypes
import os

import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "paritytech-bn_amd", "libbn254mi.so")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB), "libbn254mi.so not built (run __graft_entry__.build())"
    return _native.load()


def test_every_new_entry_point_refuses_a_null_context(lib):
    buf = np.zeros(64, np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    off = np.array([0, 1], np.uintp)
    po = ctypes.c_void_p(off.ctypes.data)
    INVALID = _native.BN_ERR_INVALID_ARGUMENT
    assert lib.bn_g1_msm_many(None, p, p, po, 1, p, 1) == INVALID
    assert lib.bn_g1_msm_many_dev(None, p, p, po, 1, p, 1, None) == INVALID
    assert lib.bn_g1_msm_many(None, None, None, None, 0, None, 1) == INVALID
    for v in (0, 4):
        assert lib.bn_set_msm_many_window(None, v) == INVALID
        assert lib.bn_set_msm_many_unit(None, v) == INVALID
        assert lib.bn_set_msm_many_max(None, v) == INVALID
        assert lib.bn_set_msm_many_chunk(None, v) == INVALID
    assert lib.bn_g1_msm_many_reserve(None, 16, 4) == INVALID
    assert not buf.any()


class _Lib:
    """Stands in for the native library: records the calls it is handed."""

    def __init__(self):
        self.calls = []

    def bn_g1_msm_many(self, h, p, k, off, m, out, out_stride):
        o = np.ctypeslib.as_array(ctypes.cast(off, ctypes.POINTER(ctypes.c_size_t)), shape=(m + 1,)).copy()
        n = int(o[-1])
        kk = np.ctypeslib.as_array(ctypes.cast(k, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 4)).copy() if n else None
        pp = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 12)).copy() if n else None
        self.calls.append({"off": o, "m": m, "stride": out_stride, "k": kk, "p": pp})
        return _native.BN_OK

    def bn_g1_msm_many_dev(self, h, d_p, d_k, off, m, d_out, out_stride, stream):
        o = np.ctypeslib.as_array(ctypes.cast(off, ctypes.POINTER(ctypes.c_size_t)), shape=(m + 1,)).copy()
        self.calls.append({"off": o, "m": m, "stride": out_stride, "dev": True})
        return _native.BN_OK


def _ctx():
    c = _native.Context.__new__(_native.Context)
    c._h = ctypes.c_void_p(1)
    c._L = _Lib()
    c._owner = c      # close() then leaves the stub's fake context handle alone
    return c


def test_segments_reach_the_library_flat_with_their_offsets():
    c = _ctx()
    g, f = bn.G1.one(), bn.Fr.from_int
    msms = [([g, g], [f(3), f(4)]), ([], []), ([g], [f(5)])]
    out = bn.g1_msm_many(msms, ctx=c)
    assert len(out) == 3 and all(isinstance(x, bn.G1) for x in out)
    (call,) = c._L.calls
    assert call["m"] == 3 and call["stride"] == 1 and list(call["off"]) == [0, 2, 2, 3]
    assert np.array_equal(call["k"], np.stack([f(3).img, f(4).img, f(5).img]))
    assert np.array_equal(call["p"], np.stack([g.img, g.img, g.img]))
    # the image-array forms, a stride, and only empty segments (NULL p and k)
    p, k = np.zeros((3, 12), np.uint64), np.zeros((3, 4), np.uint64)
    assert c.g1_msm_many(p, k, [0, 3], out_stride=2).shape == (2, 12)
    assert c._L.calls[1]["stride"] == 2
    assert c.g1_msm_many(p[:0], k[:0], [0, 0, 0]).shape == (2, 12) and c._L.calls[2]["p"] is None
    c.g1_msm_many_dev(0x1000, 0x2000, [0, 1, 3], 0x3000, 2)
    assert c._L.calls[3]["m"] == 2 and c._L.calls[3]["stride"] == 2 and list(c._L.calls[3]["off"]) == [0, 1, 3]


def test_the_empty_call_makes_no_native_call():
    c = _ctx()
    assert bn.g1_msm_many([], ctx=c) == []
    assert c.g1_msm_many(np.zeros((0, 12), np.uint64), np.zeros((0, 4), np.uint64), [0]).shape == (0, 12)
    assert c._L.calls == []


def test_argument_errors_are_raised_before_any_native_call():
    c = _ctx()
    g, one = bn.G1.one(), bn.Fr.from_int(1)
    p, k = np.zeros((3, 12), np.uint64), np.zeros((3, 4), np.uint64)
    with pytest.raises(ValueError):
        bn.g1_msm_many([([g, g], [one])], ctx=c)                   # two points, one scalar
    with pytest.raises(ValueError):
        c.g1_msm_many(p, k[:2], [0, 3])
    for off in ([0, 2], [1, 3], [0, 2, 1, 3], [], [[0, 3]], [0.0, 3.0], [0, -1, 3]):
        with pytest.raises(ValueError):
            c.g1_msm_many(p, k, off)
    with pytest.raises(ValueError):
        c.g1_msm_many(p, k, [0, 3], out_stride=0)
    with pytest.raises(ValueError):
        c.g1_msm_many_dev(0, 0, [0, 3], 0, out_stride=0)
    with pytest.raises(ValueError):
        c.g1_msm_many_dev(0, 0, [0, 3, 2], 0)
    assert c._L.calls == []


def test_native_mirror_lists_the_new_entry_points():
    for name in ("bn_g1_msm_many", "bn_g1_msm_many_dev", "bn_set_msm_many_window", "bn_set_msm_many_unit",
                 "bn_set_msm_many_max", "bn_set_msm_many_chunk", "bn_g1_msm_many_reserve"):
        assert name in _native.EXPORTS
    for m in ("g1_msm_many", "g1_msm_many_dev", "set_msm_many_window", "set_msm_many_unit", "set_msm_many_max",
              "set_msm_many_chunk", "g1_msm_many_reserve"):
        assert callable(getattr(_native.Context, m))
    assert callable(bn.g1_msm_many)
