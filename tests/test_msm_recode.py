"""The signed-window recoding and the (window, bucket) keys of the G1 multi-scalar
multiplication (csrc/msm.h), compiled for the host: for every supported window
width c, sum d_w * 2^(c*w) == k, |d_w| <= 2^(c-1), exactly W(c) digits and no carry
out of the top window -- for the scalars where a recoding goes wrong: 0, 1, 2,
r-1, r-2, every 2^j and 2^j - 1, 2^(c-1) and its neighbours in every window
position, the all-ones pattern (a carry through every window) and random scalars."""
import numpy as np
import pytest

from tests.native import msmemul

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def _widths():
    L = msmemul.lib()
    return list(range(L.msm_emul_min_window(), L.msm_emul_max_window() + 1))


def _scalars(c):
    s = [0, 1, 2, R - 1, R - 2]
    for j in range(254):
        s += [1 << j, (1 << j) - 1]
    half = 1 << (c - 1)
    w = 0
    while c * w < 254:
        for v in (half - 1, half, half + 1):
            s.append((v << (c * w)) % R)
        w += 1
    s.append((1 << 253) - 1)  # all ones below r: raw windows of 2^c - 1, a carry through every window
    s.append(((1 << 254) - 1) % R)
    rng = np.random.default_rng(20240 + c)
    for _ in range(500):
        s.append(int.from_bytes(rng.bytes(32), "little") % R)
    assert all(0 <= v < R for v in s)
    return s


def test_supported_range():
    assert _widths() == list(range(2, 17))
    L = msmemul.lib()
    assert not L.msm_emul_window_ok(1) and not L.msm_emul_window_ok(17) and not L.msm_emul_window_ok(0)
    assert L.msm_emul_max_windows() == max(L.msm_emul_windows(c) for c in _widths())


@pytest.mark.parametrize("c", list(range(2, 17)))
def test_recoding(c):
    L = msmemul.lib()
    nw = L.msm_emul_windows(c)
    # W(c): the fewest windows whose top one can absorb the carry for every k < 2^254,
    # i.e. c * W >= 255 (a top window of at most c - 1 scalar bits)
    assert c * nw >= 255 and c * (nw - 1) < 255
    assert L.msm_emul_buckets(c) == 1 << (c - 1)
    assert L.msm_emul_num_keys(c) == nw << (c - 1)
    ks = _scalars(c)
    d, carry = msmemul.recode(ks, c)
    assert d.shape == (len(ks), nw)
    assert carry == 0
    half = 1 << (c - 1)
    assert int(np.abs(d.astype(np.int64)).max()) <= half
    for k, row in zip(ks, d):
        assert sum(int(v) << (c * w) for w, v in enumerate(row)) == k
    # the top window's digit is never negative and fits the bits it holds plus the carry
    top = d[:, nw - 1]
    assert int(top.min()) >= 0 and int(top.max()) <= 1 << L.msm_emul_top_bits(c)
    # the all-ones scalar really carries through every window below the top
    ones = d[ks.index((1 << 253) - 1)]
    assert ones[0] == -1 and (ones[1:(253 // c)] == 0).all()


@pytest.mark.parametrize("c", list(range(2, 17)))
def test_key_mapping(c):
    """key -> (window, weight) inverts (window, |d|) -> key for every term index; the top
    window (t scalar bits, digits 0 .. 2^t) spreads each digit over 2^(c-1-t) replicas by
    the term's index, every other window has one bucket per digit"""
    L = msmemul.lib()
    nw, nb = L.msm_emul_windows(c), 1 << (c - 1)
    t = L.msm_emul_top_bits(c)
    assert t == 254 - c * (nw - 1) and 0 <= t <= c - 1
    indices = (0, 1, 2, 5, nb - 1, nb, 12345, (1 << 26) - 1)
    for w in sorted({0, 1, nw // 2, nw - 2, nw - 1}):
        top = w == nw - 1
        rs = L.msm_emul_replica_shift(c, w)
        assert rs == (c - 1 - t if top else 0)
        top_mag = (1 << t) if top else nb
        keys = {}
        for m in sorted({1, min(2, top_mag), max(1, top_mag // 2), max(1, top_mag - 1), top_mag}):
            for d in ((m,) if top else (m, -m)):  # the top window's digits are never negative
                for idx in indices:
                    key = L.msm_emul_key(c, w, d, idx)
                    assert w * nb <= key < (w + 1) * nb
                    assert L.msm_emul_key_window(c, key) == w
                    assert L.msm_emul_key_weight(c, key) == m
                    keys.setdefault(m, set()).add(key)
        for m, ks in keys.items():
            assert len(ks) == len({i & ((1 << rs) - 1) for i in indices})  # one key per replica
        allk = [k for ks in keys.values() for k in ks]
        assert len(allk) == len(set(allk))  # different weights never share a bucket
    for idx in (0, 1, (1 << 26) - 1):
        for d in (3, -3):
            e = L.msm_emul_entry(idx, d)
            assert L.msm_emul_entry_index(e) == idx and bool(L.msm_emul_entry_neg(e)) == (d < 0)
