"""CPU checks of the structured vectors of tests/edge_vectors.py, before any GPU
time is spent on them: the vectors are valid and complete; the oracle is right on
them, by a second, independent reference (a Python-integer tower and pow()); and
the engine's formulas compiled for the host (tests/native/hostemul.py, built with
BN_HOST_CHECKS: a bound violation aborts) agree with the oracle bit for bit."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E
from tests.native import hostemul as H

P, R = O.P, O.R


# ---------------------------------------------------------------- generator self-checks
def test_set_sizes():
    """Hard floors: an empty or truncated set cannot pass silently."""
    assert len(E.e0(P)) >= 42 and len(E.e0(R)) >= 42
    assert len(E.gcd_sweep()) >= 550
    rows, labels, vals = E.fq12_rows()
    assert rows.shape[0] >= 140 and len(labels) == rows.shape[0] == len(vals)
    assert E.fq12_subfield_mask(labels).sum() >= 20
    assert len(E.g1_affine()) >= 60 and len(E.g2_affine()) == 16
    assert len(E.g1_z_values()) >= 120 and len(E.g2_z_values()) >= 480
    assert E.g1_rescaled()[0].shape[0] >= 120 and E.g2_rescaled()[0].shape[0] >= 480
    assert E.gcd_points()[0].shape[0] >= 550
    assert E.scalars()[0].shape[0] >= 85
    assert E.pairing_pairs()[0].shape[0] >= 380
    assert len(E.digit_boundary_values()) >= 40
    assert E.fq_elements()[0].shape[0] >= 126


def test_views_are_what_they_say():
    """image view: the memory image is v; internal view: image * 2^5 == v (mod p),
    the engine's x * 2^261 with the image's 2^256 taken out."""
    base = E.e0(P)
    img, labels, _ = E.fq_elements()
    ints = O.array_to_ints(img)
    n = len(base)
    assert [v for _, v in base] == O.mont_array_to_canon(img[:n])
    assert [v for _, v in base] == ints[n:2 * n]
    assert [v for _, v in base] == [x * 32 % P for x in ints[2 * n:]]
    assert labels[0] == "field 0" and labels[n] == "image 0" and labels[2 * n] == "internal 0"
    k, _, vals = E.scalars()
    assert O.mont_array_to_canon(k, O.FR) == vals and all(0 <= v < R for v in vals)
    assert {v for _, v in E.e0(R)} <= set(O.array_to_ints(k)) and {v for _, v in E.e0(R)} <= set(vals)


def test_x_zero_is_not_on_the_curve():
    labels = [p[0] for p in E.g1_affine()]
    assert "x=0 +y" not in labels and "x=1 +y" in labels and len(labels) == 2 * 57 + 8


def test_points_are_group_elements():
    g1, _ = E.g1_affine_jac()
    _, st = O.g1_affine_new(g1[:, :4], g1[:, 4:8])
    assert not st.any()
    g2, _ = E.g2_affine_jac()
    _, st = O.g2_affine_new(g2[:, :8], g2[:, 8:16], 8)
    assert not st.any()


def test_rescaled_points_equal_their_sources():
    for fn, eq in ((E.g1_rescaled, O.g1_eq), (E.g2_rescaled, O.g2_eq)):
        resc, src, labels = fn()
        bad = [labels[i] for i, ok in enumerate(eq(resc, src)) if not ok]
        assert not bad, bad[:5]
        w = resc.shape[1] // 3
        assert resc[:, 2 * w:].any(axis=1).all()  # no zero z
    resc, src, labels = E.gcd_points()
    assert all(O.g1_eq(resc, np.tile(src, (resc.shape[0], 1))))
    p, q, labels = E.pairing_pairs()
    assert len(labels) == p.shape[0] == q.shape[0]


def test_cross_covers_both_sets():
    for n_a, n_b in ((123, 89), (492, 89), (33, 89)):
        i, j = E.cross(n_a, n_b)
        assert len(i) <= 2000 and set(i) == set(range(n_a)) and set(j) == set(range(n_b))


# ---------------------------------------------------------------- the second reference
# Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - (9 + u)), Fq12 = Fq6[w]/(w^2 - v), on
# Python integers, schoolbook formulas (no Karatsuba, no lazy reduction).
XI = (9, 1)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2inv(a):
    t = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)  # (0 -> 0)
    return (a[0] * t % P, -a[1] * t % P)


def f6add(a, b):
    return tuple(f2add(x, y) for x, y in zip(a, b))


def f6sub(a, b):
    return tuple(f2sub(x, y) for x, y in zip(a, b))


def f6mul(a, b):
    m = lambda i, j: f2mul(a[i], b[j])  # noqa: E731
    return (f2add(m(0, 0), f2mul(XI, f2add(m(1, 2), m(2, 1)))),
            f2add(f2add(m(0, 1), m(1, 0)), f2mul(XI, m(2, 2))),
            f2add(f2add(m(0, 2), m(1, 1)), m(2, 0)))


def f6mulv(a):
    return (f2mul(XI, a[2]), a[0], a[1])


def f6inv(a):
    c0 = f2sub(f2mul(a[0], a[0]), f2mul(XI, f2mul(a[1], a[2])))
    c1 = f2sub(f2mul(XI, f2mul(a[2], a[2])), f2mul(a[0], a[1]))
    c2 = f2sub(f2mul(a[1], a[1]), f2mul(a[0], a[2]))
    t = f2inv(f2add(f2mul(a[0], c0), f2mul(XI, f2add(f2mul(a[2], c1), f2mul(a[1], c2)))))
    return (f2mul(c0, t), f2mul(c1, t), f2mul(c2, t))


def f12mul(a, b):
    return (f6add(f6mul(a[0], b[0]), f6mulv(f6mul(a[1], b[1]))), f6add(f6mul(a[0], b[1]), f6mul(a[1], b[0])))


def f12inv(a):
    t = f6inv(f6sub(f6mul(a[0], a[0]), f6mulv(f6mul(a[1], a[1]))))
    zero6 = ((0, 0),) * 3
    return (f6mul(a[0], t), f6sub(zero6, f6mul(a[1], t)))


def f12pow(a, e):
    r = (((1, 0), (0, 0), (0, 0)), ((0, 0),) * 3)
    for bit in bin(e)[2:]:
        r = f12mul(r, r)
        if bit == "1":
            r = f12mul(r, a)
    return r


def nest(c):
    return tuple(tuple((c[6 * i + 2 * j], c[6 * i + 2 * j + 1]) for j in range(3)) for i in range(2))


def flat(a):
    return [c for h in a for f2 in h for c in f2]


@pytest.fixture(scope="module")
def rows():
    return E.fq12_rows()


def test_tower_relations():
    """The Python tower itself: u^2 = -1, v^3 = 9 + u, w^2 = v, a * a^-1 = 1."""
    one = nest([1] + [0] * 11)
    w = nest([0] * 6 + [1] + [0] * 5)
    v = nest([0, 0, 1] + [0] * 9)
    assert f12mul(w, w) == v
    assert flat(f12mul(f12mul(v, v), v)) == [9, 1] + [0] * 10
    a = nest(E.filler(12, salt=9))
    assert f12mul(a, f12inv(a)) == one and f12mul(a, one) == a


def test_oracle_fq12_against_python_tower(rows):
    arr, labels, vals = rows
    n = arr.shape[0]
    rot = np.roll(arr, -1, axis=0)
    mul = O.binary("orc_fq12_mul", arr, rot, 48, 48, 48)
    sqr = O.unary("orc_fq12_squared", arr, 48)[0]
    inv, rcs = O.unary("orc_fq12_inverse", arr, 48)
    for k in range(n):
        a, b = nest(vals[k]), nest(vals[(k + 1) % n])
        assert O.mont_array_to_canon(mul[k]) == flat(f12mul(a, b)), labels[k]
        assert O.mont_array_to_canon(sqr[k]) == flat(f12mul(a, a)), labels[k]
        assert O.mont_array_to_canon(inv[k]) == flat(f12inv(a)), labels[k]
    assert not inv[0].any()  # zero -> None, the output stays zero


def test_oracle_frobenius_is_the_pth_power(rows):
    arr, labels, vals = rows
    pick = [1, 2, 9, 20, 30, 40, arr.shape[0] // 2, arr.shape[0] - 1]
    for k in pick:
        want = np.zeros(48, np.uint64)
        O.lib().orc_fq12_frobenius_map(O._p(np.ascontiguousarray(arr[k])), 1, O._p(want))
        assert O.mont_array_to_canon(want) == flat(f12pow(nest(vals[k]), P)), labels[k]


def test_oracle_inversion_on_the_gcd_sweep():
    """g1_normalize of the point at z = u_g (mod.rs:199-226: one Fq inversion per
    point) against pow(z, -1, p), for the whole of GCD(p)."""
    resc, src, labels = E.gcd_points()
    got = O.g1_normalize(resc)
    one = O.to_mont(1)
    for k in range(resc.shape[0]):
        x, y, z = O.mont_array_to_canon(resc[k])
        zi = pow(z, -1, P)
        want = [O.to_mont(x * zi * zi), O.to_mont(y * zi * zi * zi), one]
        assert O.array_to_ints(got[k]) == want, labels[k]
    assert np.array_equal(got, np.tile(src, (resc.shape[0], 1)))


def test_oracle_sqrt_on_e0():
    a, labels, vals = E.fq_elements()
    out, ok = O.fq_sqrt(a)
    roots = O.mont_array_to_canon(out)
    for k, v in enumerate(vals):
        is_sq = v == 0 or pow(v, (P - 1) // 2, P) == 1
        assert bool(ok[k]) == is_sq, labels[k]
        if is_sq:
            assert roots[k] * roots[k] % P == v, labels[k]


# ---------------------------------------------------------------- host emulation vs the oracle
def _frob(a, pw):
    out = np.zeros(48, np.uint64)
    O.lib().orc_fq12_frobenius_map(O._p(np.ascontiguousarray(a)), pw, O._p(out))
    return out


def test_host_fq12_ops_on_structured_rows(rows):
    arr, labels, _ = rows
    n = arr.shape[0]
    rot = np.roll(arr, -1, axis=0)
    want = {
        "he_fq12_mul": O.binary("orc_fq12_mul", arr, rot, 48, 48, 48),
        "he_fq12_sqr": O.unary("orc_fq12_squared", arr, 48)[0],
        "he_fq12_inv": O.unary("orc_fq12_inverse", arr, 48)[0],
        "he_fq12_cyc_sqr": O.unary("orc_fq12_cyclotomic_squared", arr, 48)[0],
        "he_fq12_exp_by_neg_z": O.unary("orc_fq12_exp_by_neg_z", arr, 48)[0],
    }
    for k in range(n):
        for name, w in want.items():
            args = (arr[k], rot[k]) if name == "he_fq12_mul" else (arr[k],)
            assert np.array_equal(H.call(name, *args, out_words=96), w[k]), (name, labels[k])
        for pw in (1, 2, 3):
            assert np.array_equal(H.call("he_fq12_frob", arr[k], out_words=96, ints=(pw,)), _frob(arr[k], pw)), \
                (pw, labels[k])


def test_host_final_exp_on_subfield_rows(rows):
    arr, labels, _ = rows
    sub = E.fq12_subfield_mask(labels)
    sub |= np.array([lab.startswith("c0 = 0") for lab in labels])
    want, rcs = O.final_exponentiation(arr[sub])
    one = O.canon_to_mont_array([1] + [0] * 11)
    for j, k in enumerate(np.flatnonzero(sub)):
        assert rcs[j] == 0
        assert np.array_equal(H.call("he_final_exp", arr[k], out_words=96), want[j]), labels[k]
        if not labels[k].startswith("c0 = 0"):
            assert np.array_equal(want[j], one), labels[k]


def test_host_gt_pow_on_the_scalar_set():
    p, q, _ = E.pairing_pairs()
    one = O.canon_to_mont_array([1] + [0] * 11)
    minus = O.canon_to_mont_array([P - 1] + [0] * 11)
    a = np.stack([one, minus, O.pairing_many(p[7:8], q[7:8])[0]])
    k, labels, vals = E.scalars()
    for j in range(3):
        want = O.gt_pow(np.tile(a[j], (len(vals), 1)), k)
        for s, v in enumerate(vals):
            words = np.frombuffer(int(v).to_bytes(32, "little"), np.uint64).copy()
            got = H.call("he_gt_pow", a[j], words, out_words=96)
            assert np.array_equal(got, want[s]), (j, labels[s])


def test_host_group_mul_on_structured_points():
    k, klabels, kvals = E.scalars()
    p1, _, l1 = E.g1_rescaled()
    p2, _, l2 = E.g2_rescaled()
    for t in range(24):
        i1, i2, s = (t * 5) % p1.shape[0], (t * 21) % p2.shape[0], (t * 4) % len(kvals)
        kc = O.ints_to_array([kvals[s]])
        assert np.array_equal(H.call("he_g1_mul", p1[i1], kc, out_words=24), O.g1_mul(p1[i1], k[s])[0]), \
            (l1[i1], klabels[s])
        assert np.array_equal(H.call("he_g2_mul", p2[i2], kc, out_words=48), O.g2_mul(p2[i2], k[s])[0]), \
            (l2[i2], klabels[s])


def _he_rc(name, inp, out_words):
    fn = getattr(H.lib(), name)
    fn.restype = ctypes.c_int
    inp = np.ascontiguousarray(inp)
    out = np.zeros(out_words, dtype=np.uint32)
    rc = fn(inp.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return out.view(np.uint64), rc


def test_host_sqrt_on_e0():
    a, labels, _ = E.fq_elements()
    ref, ok = O.fq_sqrt(a)
    for k in range(a.shape[0]):
        got, some = _he_rc("he_fq_sqrt", a[k].view(np.uint32), 8)
        assert bool(some) == bool(ok[k]), labels[k]
        if some:
            assert np.array_equal(got, ref[k]), labels[k]
    # Fq2: (v, 0), (0, v), and (v, next v)
    n = a.shape[0]
    a2 = np.concatenate([np.concatenate([a, np.zeros_like(a)], axis=1), np.concatenate([np.zeros_like(a), a], axis=1),
                         np.concatenate([a, np.roll(a, -1, axis=0)], axis=1)])
    ref, ok = O.fq2_sqrt(a2)
    for k in range(a2.shape[0]):
        got, some = _he_rc("he_fq2_sqrt", a2[k].view(np.uint32), 16)
        assert bool(some) == bool(ok[k]), (k // n, labels[k % n])
        if some:
            assert np.array_equal(got, ref[k]), (k // n, labels[k % n])
