"""Argument handling of substrate_bn.g2_msm (the Python mirror of bn_g2_msm) that
needs no device: the accepted input forms, the length check and the empty sum."""
import numpy as np
import pytest

import substrate_bn as bn


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to reach the engine fails the test."""
    def boom():
        raise AssertionError("g2_msm reached the device")
    monkeypatch.setattr(bn, "context", boom)


def test_empty_sum_is_zero_without_a_device_call(no_device):
    for pts, ks in (([], []), (np.zeros((0, 24), np.uint64), np.zeros((0, 4), np.uint64)), ((), iter(()))):
        out = bn.g2_msm(pts, ks)
        assert isinstance(out, bn.G2) and out.same_image(bn.G2.zero()) and out.is_zero()


def test_mismatched_lengths_raise(no_device):
    one, k = bn.G2.one(), bn.Fr.from_int(5)
    with pytest.raises(ValueError):
        bn.g2_msm([one, one], [k])
    with pytest.raises(ValueError):
        bn.g2_msm([], [k])
    with pytest.raises(ValueError):
        bn.g2_msm(np.zeros((3, 24), np.uint64), np.zeros((2, 4), np.uint64))
    with pytest.raises(ValueError):  # not whole rows
        bn.g2_msm(np.zeros(25, np.uint64), np.zeros(4, np.uint64))
    with pytest.raises(ValueError):  # G1 rows are not G2 rows
        bn.g2_msm(np.zeros(12, np.uint64), np.zeros(4, np.uint64))


def test_sequences_and_arrays_reach_the_engine_as_the_same_rows(monkeypatch):
    seen = []

    class Ctx:
        def g2_msm(self, p, k):
            seen.append((p.copy(), k.copy()))
            return bn.G2.one().img

    monkeypatch.setattr(bn, "context", lambda: Ctx())
    pts = [bn.G2.one(), bn.G2.zero()]
    ks = [bn.Fr.from_int(7), bn.Fr.from_int(0)]
    a = bn.g2_msm(pts, ks)
    b = bn.g2_msm(np.stack([p.img for p in pts]), np.stack([k.img for k in ks]))
    assert isinstance(a, bn.G2) and a.same_image(b)
    (p0, k0), (p1, k1) = seen
    assert p0.shape == (2, 24) and k0.shape == (2, 4) and p0.dtype == np.uint64
    assert np.array_equal(p0, p1) and np.array_equal(k0, k1)


def test_native_mirror_lists_the_g2_msm_entry_points():
    from substrate_bn import _native
    for name in ("bn_g2_msm", "bn_g2_msm_dev", "bn_g2_msm_reserve"):
        assert name in _native.EXPORTS
    for m in ("g2_msm", "g2_msm_dev", "g2_msm_reserve", "set_msm_window", "set_msm_min"):
        assert callable(getattr(_native.Context, m))
