"""Argument handling of pairing_batch_many (the Python mirror of bn_pairing_batch_many)
that needs no device: the empty list, the offsets built from nested sequences, the
offsets the array form refuses, and the listings of the new entry points."""
import numpy as np
import pytest

import substrate_bn as bn
from substrate_bn import _native


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to reach the engine fails the test."""
    def boom():
        raise AssertionError("pairing_batch_many reached the device")
    monkeypatch.setattr(bn, "context", boom)


class _Lib:
    """Stands in for the native library: records the call, fills the rows with their index."""

    def __init__(self):
        self.calls = []

    def bn_pairing_batch_many(self, h, p, q, off, m, out):
        self.calls.append(("host", m))
        return _native.BN_OK

    def bn_pairing_batch_many_dev(self, h, p, q, off, m, out, stream):
        self.calls.append(("dev", m))
        return _native.BN_OK


def _ctx():
    c = _native.Context.__new__(_native.Context)
    c._h = None
    c._L = _Lib()
    return c


def test_no_products_give_an_empty_list_without_a_device_call(no_device):
    assert bn.pairing_batch_many([]) == []
    assert bn.pairing_batch_many(()) == []
    assert bn.pairing_batch_many(iter(())) == []


def test_nested_sequences_reach_the_engine_as_rows_and_offsets(monkeypatch):
    seen = []

    class Ctx:
        def pairing_batch_many(self, p, q, offsets):
            seen.append((p.copy(), q.copy(), np.array(offsets)))
            return np.stack([np.full(48, j, np.uint64) for j in range(len(offsets) - 1)])

    monkeypatch.setattr(bn, "context", lambda: Ctx())
    a, b, z1, z2 = bn.G1.one(), bn.G2.one(), bn.G1.zero(), bn.G2.zero()
    out = bn.pairing_batch_many([[(a, b), (z1, b)], [], ((a, z2),), iter([(a, b), (a, b), (z1, z2)]), []])
    (p, q, off), = seen
    assert [int(v) for v in off] == [0, 2, 2, 3, 6, 6]
    assert p.shape == (6, 12) and q.shape == (6, 24) and p.dtype == np.uint64 and q.dtype == np.uint64
    assert np.array_equal(p, np.stack([x.img for x in (a, z1, a, a, a, z1)]))
    assert np.array_equal(q, np.stack([x.img for x in (b, b, z2, b, b, z2)]))
    assert len(out) == 5 and all(isinstance(g, bn.Gt) for g in out)
    assert [int(g.img[0]) for g in out] == [0, 1, 2, 3, 4]


def test_only_empty_products_pass_zero_rows(monkeypatch):
    seen = []

    class Ctx:
        def pairing_batch_many(self, p, q, offsets):
            seen.append((p.shape, q.shape, [int(v) for v in offsets]))
            return np.stack([bn.Gt.one().img] * (len(offsets) - 1))

    monkeypatch.setattr(bn, "context", lambda: Ctx())
    out = bn.pairing_batch_many([[], []])
    assert seen == [((0, 12), (0, 24), [0, 0, 0])]
    assert out == [bn.Gt.one(), bn.Gt.one()]


def test_array_form_passes_sound_offsets():
    c = _ctx()
    p, q = np.zeros((5, 12), np.uint64), np.zeros((5, 24), np.uint64)
    out = c.pairing_batch_many(p, q, [0, 2, 2, 5])
    assert out.shape == (3, 48) and out.dtype == np.uint64
    out = c.pairing_batch_many(p[:0], q[:0], np.zeros(1, np.int64))          # no products
    assert out.shape == (0, 48)
    c.pairing_batch_many_dev(0, 0, (0, 0, 4), 0)
    assert c._L.calls == [("host", 3), ("host", 0), ("dev", 2)]


@pytest.mark.parametrize("offsets", [
    [0, 3, 2, 5],            # decreasing
    [0, 5, 4],               # decreasing at the end
    [1, 2, 5],               # nonzero first offset
    [0, 2, 4],               # wrong length: ends before the last pair
    [0, 2, 6],               # wrong length: ends past the last pair
    [],                      # not even offsets[0]
    [[0, 5]],                # not one-dimensional
    [0, -1, 5],              # negative
    [0.0, 2.5, 5.0],         # not integers
])
def test_malformed_offsets_raise_before_any_native_call(offsets):
    c = _ctx()
    p, q = np.zeros((5, 12), np.uint64), np.zeros((5, 24), np.uint64)
    with pytest.raises(ValueError):
        c.pairing_batch_many(p, q, offsets)
    assert c._L.calls == []


def test_dev_form_checks_its_host_offsets():
    c = _ctx()
    for offsets in ([0, 3, 2], [1, 2], []):
        with pytest.raises(ValueError):
            c.pairing_batch_many_dev(0, 0, offsets, 0)
    assert c._L.calls == []


def test_mismatched_rows_raise():
    c = _ctx()
    with pytest.raises(ValueError):
        c.pairing_batch_many(np.zeros((3, 12), np.uint64), np.zeros((2, 24), np.uint64), [0, 3])
    assert c._L.calls == []


def test_native_mirror_lists_the_entry_points():
    for name in ("bn_pairing_batch_many", "bn_pairing_batch_many_dev", "bn_set_products_min",
                 "bn_set_products_chunk"):
        assert name in _native.EXPORTS
    for m in ("pairing_batch_many", "pairing_batch_many_dev", "set_products_min", "set_products_chunk"):
        assert callable(getattr(_native.Context, m))
    assert callable(bn.pairing_batch_many)
