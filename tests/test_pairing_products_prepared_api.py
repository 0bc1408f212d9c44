"""Argument handling of pairing_batch_prepared_many in the Python mirror (over
bn_pairing_batch_prepared_many) that needs no device, with a stub in place of the native
library: the compacted q holds only the fresh terms' points in term order, the qidx array is
uint32 with 0xffffffff at the fresh terms, the offsets come from the product lengths, a bad
index, a product of 65 terms and a closed handle are refused in Python with no native call,
the empty call makes none, and the new names are listed."""
import ctypes

import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native

HANDLE = 0x5150
FRESH = 0xFFFFFFFF


class _Lib:
    """Stands in for the native library: records what each call was handed."""

    def __init__(self, nq):
        self.nq = nq
        self.calls = []

    def bn_g2_prepare(self, h, q, nq, out):
        out._obj.value = HANDLE
        return _native.BN_OK

    def bn_g2_prepared_count(self, handle):
        return self.nq

    def bn_g2_prepared_destroy(self, h, handle):
        return _native.BN_OK

    def bn_pairing_batch_prepared_many(self, h, p, q, handle, qidx, offsets, m, out):
        off = np.ctypeslib.as_array(ctypes.cast(offsets, ctypes.POINTER(ctypes.c_size_t)), shape=(m + 1,)).copy()
        n = int(off[-1])
        raw = np.ctypeslib.as_array(ctypes.cast(qidx, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)) if n else \
            np.zeros(0, np.uint32)
        ix = raw.copy()
        nf = int((ix == FRESH).sum())
        pp = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n, 12)).copy() if n else None
        qq = np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_uint64)), shape=(nf, 24)).copy() if nf else None
        self.calls.append({"handle": handle, "off": off, "qidx": ix, "qidx_dtype": raw.dtype, "p": pp, "q": qq, "m": m,
                           "q_null": not q})
        return _native.BN_OK


def _prepared(nq):
    c = _native.Context.__new__(_native.Context)
    c._h = ctypes.c_void_p(1)
    c._L = _Lib(nq)
    c._owner = c      # close() then leaves the stub's fake context handle alone
    return c, bn.G2Prepared([bn.G2.one()] * nq, ctx=c)


def _g2(k):
    """A G2 value with a recognisable image (never sent to a device)."""
    return bn.G2(np.arange(24, dtype=np.uint64) + np.uint64(100 * k))


def _g1(k):
    return bn.G1(np.arange(12, dtype=np.uint64) + np.uint64(1000 * k))


def test_fresh_points_are_compacted_in_term_order_and_indices_are_uint32():
    c, prep = _prepared(3)
    products = [[(_g1(0), _g2(0)), (_g1(1), 0), (_g1(2), 1), (_g1(3), 2)],
                [],
                [(_g1(4), 2), (_g1(5), _g2(5))],
                [(_g1(6), _g2(6)), (_g1(7), _g2(7))],
                [(_g1(8), np.int64(1))]]
    out = bn.pairing_batch_prepared_many(products, prep)
    assert len(out) == 5 and all(isinstance(g, bn.Gt) for g in out)
    (call,) = c._L.calls
    assert call["handle"] == HANDLE and call["m"] == 5
    assert [int(v) for v in call["off"]] == [0, 4, 4, 6, 8, 9]          # from the product lengths
    assert call["qidx_dtype"] == np.uint32
    assert [int(v) for v in call["qidx"]] == [FRESH, 0, 1, 2, 2, FRESH, FRESH, FRESH, 1]
    assert np.array_equal(call["p"], np.stack([_g1(k).img for k in range(9)]))
    assert np.array_equal(call["q"], np.stack([_g2(k).img for k in (0, 5, 6, 7)]))   # only the fresh ones


def test_all_prepared_products_pass_a_null_q():
    c, prep = _prepared(2)
    bn.pairing_batch_prepared_many([[(_g1(0), 0), (_g1(1), 1)]], prep)
    (call,) = c._L.calls
    assert call["q_null"] and call["q"] is None
    assert [int(v) for v in call["qidx"]] == [0, 1]


@pytest.mark.parametrize("bad", [3, -1, 0xFFFFFFFF, 0xFFFFFFFE, 1 << 32])
def test_a_bad_index_is_refused_before_the_call(bad):
    c, prep = _prepared(3)
    with pytest.raises(ValueError):
        bn.pairing_batch_prepared_many([[(_g1(0), _g2(0)), (_g1(1), bad)]], prep)
    assert c._L.calls == []


def test_a_product_of_65_terms_is_refused_before_the_call():
    c, prep = _prepared(1)
    bn.pairing_batch_prepared_many([[(_g1(0), 0)] * 64], prep)
    assert len(c._L.calls) == 1
    with pytest.raises(ValueError):
        bn.pairing_batch_prepared_many([[(_g1(0), 0)], [(_g1(0), 0)] * 65], prep)
    assert len(c._L.calls) == 1


def test_a_closed_handle_is_refused_before_the_call():
    c, prep = _prepared(2)
    prep.close()
    for products in ([[(_g1(0), 0)]], []):
        with pytest.raises(ValueError):
            bn.pairing_batch_prepared_many(products, prep)
    assert c._L.calls == []


def test_no_products_give_an_empty_list_without_a_native_call():
    c, prep = _prepared(2)
    assert bn.pairing_batch_prepared_many([], prep) == []
    assert c.pairing_batch_prepared_many(np.zeros((0, 12), np.uint64), None, HANDLE, [], [0]).shape == (0, 48)
    assert c.pairing_batch_prepared_many_dev(0, 0, HANDLE, [], [0], 0) is None
    assert c._L.calls == []


def test_the_context_method_checks_its_arrays_too():
    c, _ = _prepared(4)
    p = np.zeros((3, 12), np.uint64)
    q1 = np.zeros((1, 24), np.uint64)
    assert c.pairing_batch_prepared_many(p, q1, HANDLE, [FRESH, 3, 0], [0, 1, 3]).shape == (2, 48)
    for qidx, q, off in (([FRESH, 4, 0], q1, [0, 1, 3]),            # index == nq
                         ([FRESH, 3], q1, [0, 1, 3]),               # one entry per term
                         ([FRESH, FRESH, 0], q1, [0, 1, 3]),        # q rows != fresh terms
                         ([FRESH, 3, 0], q1, [0, 1, 2]),            # offsets do not end at n
                         ([FRESH, 3, 0], q1, [1, 2, 3])):           # offsets not from 0
        with pytest.raises(ValueError):
            c.pairing_batch_prepared_many(p, q, HANDLE, qidx, off)
    assert len(c._L.calls) == 1


def test_native_mirror_lists_the_entry_points():
    for name in ("bn_pairing_batch_prepared_many", "bn_pairing_batch_prepared_many_dev"):
        assert name in _native.EXPORTS
    for m in ("pairing_batch_prepared_many", "pairing_batch_prepared_many_dev"):
        assert callable(getattr(_native.Context, m))
    assert callable(bn.pairing_batch_prepared_many)
    assert _native.QIDX_FRESH == FRESH
