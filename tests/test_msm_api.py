"""Argument handling of substrate_bn.g1_msm (the Python mirror of bn_g1_msm) that
needs no device: the accepted input forms, the length check and the empty sum."""
import numpy as np
import pytest

import substrate_bn as bn


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to reach the engine fails the test."""
    def boom():
        raise AssertionError("g1_msm reached the device")
    monkeypatch.setattr(bn, "context", boom)


def test_empty_sum_is_zero_without_a_device_call(no_device):
    for pts, ks in (([], []), (np.zeros((0, 12), np.uint64), np.zeros((0, 4), np.uint64)), ((), iter(()))):
        out = bn.g1_msm(pts, ks)
        assert isinstance(out, bn.G1) and out.same_image(bn.G1.zero()) and out.is_zero()


def test_mismatched_lengths_raise(no_device):
    one, k = bn.G1.one(), bn.Fr.from_int(5)
    with pytest.raises(ValueError):
        bn.g1_msm([one, one], [k])
    with pytest.raises(ValueError):
        bn.g1_msm([], [k])
    with pytest.raises(ValueError):
        bn.g1_msm(np.zeros((3, 12), np.uint64), np.zeros((2, 4), np.uint64))
    with pytest.raises(ValueError):  # not whole rows
        bn.g1_msm(np.zeros(13, np.uint64), np.zeros(4, np.uint64))


def test_sequences_and_arrays_reach_the_engine_as_the_same_rows(monkeypatch):
    seen = []

    class Ctx:
        def g1_msm(self, p, k):
            seen.append((p.copy(), k.copy()))
            return bn.G1.one().img

    monkeypatch.setattr(bn, "context", lambda: Ctx())
    pts = [bn.G1.one(), bn.G1.zero()]
    ks = [bn.Fr.from_int(7), bn.Fr.from_int(0)]
    a = bn.g1_msm(pts, ks)
    b = bn.g1_msm(np.stack([p.img for p in pts]), np.stack([k.img for k in ks]))
    assert isinstance(a, bn.G1) and a.same_image(b)
    (p0, k0), (p1, k1) = seen
    assert p0.shape == (2, 12) and k0.shape == (2, 4) and p0.dtype == np.uint64
    assert np.array_equal(p0, p1) and np.array_equal(k0, k1)


def test_native_mirror_lists_the_msm_entry_points():
    from substrate_bn import _native
    for name in ("bn_g1_msm", "bn_g1_msm_dev", "bn_set_msm_window", "bn_set_msm_min", "bn_msm_reserve"):
        assert name in _native.EXPORTS
    for m in ("g1_msm", "g1_msm_dev", "set_msm_window", "set_msm_min", "msm_reserve"):
        assert callable(getattr(_native.Context, m))
