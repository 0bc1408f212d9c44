"""Argument handling of the prepared-G2 calls in the Python mirror (G2Prepared,
pairing_prepared_many, miller_loop_prepared_many over bn_g2_prepare and
bn_pairing_prepared_many) that needs no device, with a stub in place of the native library:
a NULL index for idx=None, a contiguous uint32 array for a sequence, indices refused in
Python before the call, the empty batch, a closed handle, and the listings of the new names."""
import ctypes

import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native

HANDLE = 0x5150


class _Lib:
    """Stands in for the native library: records each call with the index it was handed
    (None for a NULL pointer, else a copy of the n uint32 it points at)."""

    def __init__(self, nq):
        self.nq = nq
        self.calls = []

    def bn_g2_prepare(self, h, q, nq, out):
        self.calls.append(("prepare", nq))
        out._obj.value = HANDLE
        return _native.BN_OK

    def bn_g2_prepared_count(self, handle):
        return self.nq

    def bn_g2_prepared_destroy(self, h, handle):
        self.calls.append(("destroy", handle))
        return _native.BN_OK

    def _many(self, name, handle, idx, n):
        if idx is not None:
            idx = np.ctypeslib.as_array(ctypes.cast(idx, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).copy()
        self.calls.append((name, handle, idx, n))
        return _native.BN_OK

    def bn_pairing_prepared_many(self, h, p, handle, idx, n, out):
        return self._many("pairing", handle, idx, n)

    def bn_miller_loop_prepared_many(self, h, p, handle, idx, n, out):
        return self._many("miller", handle, idx, n)


def _ctx(nq):
    c = _native.Context.__new__(_native.Context)
    c._h = ctypes.c_void_p(1)
    c._L = _Lib(nq)
    c._owner = c      # close() then leaves the stub's fake context handle alone
    return c


def _prepared(nq):
    c = _ctx(nq)
    return c, bn.G2Prepared([bn.G2.one()] * nq, ctx=c)


def test_building_passes_the_images_and_len_counts_them():
    c, prep = _prepared(3)
    assert c._L.calls == [("prepare", 3)]
    assert len(prep) == 3 and not prep.closed


@pytest.mark.parametrize("fn,name", [(bn.pairing_prepared_many, "pairing"), (bn.miller_loop_prepared_many, "miller")])
def test_idx_none_passes_a_null_index(fn, name):
    c, prep = _prepared(2)
    out = fn([bn.G1.one(), bn.G1.zero()], prep)
    assert c._L.calls[1:] == [(name, HANDLE, None, 2)]
    assert len(out) == 2 and all(isinstance(g, bn.Gt) for g in out)


@pytest.mark.parametrize("idx", [[2, 0, 1], (2, 0, 1), iter([2, 0, 1]), np.array([2, 0, 1], np.int64),
                                 np.array([9, 2, 9, 0, 9, 1], np.uint16)[1::2]])
def test_a_sequence_becomes_a_contiguous_uint32_array(idx):
    c, prep = _prepared(3)
    bn.pairing_prepared_many([bn.G1.one()] * 3, prep, idx)
    (name, handle, got, n), = c._L.calls[1:]
    assert (name, handle, n) == ("pairing", HANDLE, 3)
    assert got.dtype == np.uint32 and [int(v) for v in got] == [2, 0, 1]


@pytest.mark.parametrize("idx", [[0, 3, 1], [3, 3, 3], [0, -1, 1], [0, 1], [0, 1, 2, 0], [0.0, 1.0, 2.0], [[0, 1, 2]],
                                 [0, 1 << 32, 1]])
@pytest.mark.parametrize("fn", [bn.pairing_prepared_many, bn.miller_loop_prepared_many])
def test_bad_indices_are_refused_before_the_call(fn, idx):
    c, prep = _prepared(3)
    with pytest.raises(ValueError):
        fn([bn.G1.one()] * 3, prep, idx)
    assert c._L.calls == [("prepare", 3)]


def test_the_context_methods_check_the_indices_too():
    c = _ctx(4)
    p = np.zeros((2, 12), np.uint64)
    assert c.pairing_prepared_many(p, HANDLE, [3, 0]).shape == (2, 48)
    for bad in ([4, 0], [-1, 0], [0]):
        with pytest.raises(ValueError):
            c.pairing_prepared_many(p, HANDLE, bad)
        with pytest.raises(ValueError):
            c.miller_loop_prepared_many(p, HANDLE, bad)
    assert [call[0] for call in c._L.calls] == ["pairing"]


def test_no_pairs_give_an_empty_list_without_a_device_call():
    c, prep = _prepared(2)
    assert bn.pairing_prepared_many([], prep) == []
    assert bn.miller_loop_prepared_many((), prep, []) == []
    assert bn.pairing_prepared_many(np.zeros((0, 12), np.uint64), prep, None) == []
    assert c._L.calls == [("prepare", 2)]


def test_a_closed_handle_is_refused_and_released_once():
    c, prep = _prepared(2)
    with prep as same:
        assert same is prep
    assert prep.closed and c._L.calls[1:] == [("destroy", HANDLE)]
    prep.close()                                   # idempotent
    del same
    assert c._L.calls[1:] == [("destroy", HANDLE)]
    for fn in (bn.pairing_prepared_many, bn.miller_loop_prepared_many):
        with pytest.raises(ValueError):
            fn([bn.G1.one()], prep)
        with pytest.raises(ValueError):
            fn([], prep)
    assert c._L.calls[1:] == [("destroy", HANDLE)]


def test_dropping_the_last_reference_releases_the_handle():
    c, prep = _prepared(1)
    del prep
    import gc
    gc.collect()
    assert c._L.calls == [("prepare", 1), ("destroy", HANDLE)]


@pytest.mark.parametrize("count", [0, (1 << 16) + 1])
def test_point_counts_outside_the_limit_are_refused_in_python(count):
    c = _ctx(1)
    with pytest.raises(ValueError):
        bn.G2Prepared(np.zeros((count, 24), np.uint64), ctx=c)
    assert c._L.calls == []


def test_native_mirror_lists_the_entry_points():
    for name in ("bn_g2_prepare", "bn_g2_prepare_dev", "bn_g2_prepared_count", "bn_g2_prepared_destroy",
                 "bn_pairing_prepared_many", "bn_pairing_prepared_many_dev", "bn_miller_loop_prepared_many"):
        assert name in _native.EXPORTS
    for m in ("g2_prepare", "g2_prepare_dev", "g2_prepared_count", "g2_prepared_destroy", "pairing_prepared_many",
              "pairing_prepared_many_dev", "miller_loop_prepared_many"):
        assert callable(getattr(_native.Context, m))
    assert callable(bn.pairing_prepared_many) and callable(bn.miller_loop_prepared_many)
    assert isinstance(bn.G2Prepared, type)
