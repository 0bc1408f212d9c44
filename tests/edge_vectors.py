"""Deterministic structured operands for the edge suites (tests/test_edge_vectors.py
on the CPU, tests/test_gpu_edges.py on the MI355X): field elements, Fq12 rows,
on-curve points, Jacobian rescalings and scalars placed on the carry, borrow,
fold and zero boundaries that uniform 254-bit values never reach.

A structured integer v reaches the code in up to three views:
  "field"     the field value is v;
  "image"     the reference memory image is v (field value v * 2^-256 mod m):
              what the word-to-digit repacking and the loads and stores see;
  "internal"  Fq only: the engine's internal integer is v (field value
              v * 2^-261 mod p, fq.h: R = 2^261): what the 29-bit digits, the
              column sums, the folds and the binary GCD see.

Python integers and oracle helpers only; no randomness beyond one fixed
SplitMix64 seed for filler rows; no GPU import.  Every generator returns its
arrays with a parallel list of short labels, so that an assertion can name the
failing vector ("z: internal 2^232-1").
"""
import functools

import numpy as np

from oracle import oracle as O

P, R = O.P, O.R
M29 = (1 << 29) - 1
FILL_SEED = 0xED6E5EED
VIEWS = ("field", "image", "internal")
POW_KS = (28, 29, 30, 57, 58, 63, 64, 127, 128, 231, 232, 233, 252, 253, 254)
_MOD = {O.FQ: P, O.FR: R}
_UNVIEW = {"field": 1, "image": pow(1 << 256, -1, P), "internal": pow(1 << 261, -1, P)}
_UNVIEW_R = {"field": 1, "image": pow(1 << 256, -1, R)}


def _dedupe(items):
    """(label, value) pairs with the later copies of a value dropped."""
    seen, out = set(), []
    for lab, v in items:
        if v not in seen:
            seen.add(v)
            out.append((lab, v))
    return out


def patterns(m):
    """The three digit-pattern values below m: low eight 29-bit digits all
    0x1fffffff under the largest top digit; digits alternating 0x1fffffff, 0;
    32-bit words all 0xffffffff, masked below m."""
    low8 = (1 << 232) - 1
    top = ((m >> 232) << 232) | low8
    if top >= m:
        top -= 1 << 232
    alt = sum(M29 << (29 * i) for i in (0, 2, 4, 6))
    words = ((1 << 256) - 1) & ((1 << (m.bit_length() - 1)) - 1)
    return [("low8=1fffffff", top), ("alt 1fffffff,0", alt), ("words ffffffff", words)]


def e0(m):
    """E0(m), the base set: (label, integer) pairs, all below m, no duplicates."""
    name = "p" if m == P else "r"
    items = [("0", 0), ("1", 1), ("2", 2), ("3", 3), (name + "-1", m - 1), (name + "-2", m - 2), (name + "-3", m - 3),
             ("(%s-1)/2" % name, (m - 1) // 2), ("(%s+1)/2" % name, (m + 1) // 2), (name + "//3", m // 3)]
    for k in POW_KS:
        items.append(("2^%d" % k, (1 << k) % m))
        items.append(("2^%d-1" % k, ((1 << k) - 1) % m))
    items += patterns(m)
    assert all(0 <= v < m for _, v in items)
    return _dedupe(items)


def gcd_sweep():
    """GCD(p), the inversion sweep (the host sweep test_fq_inv_binary_gcd_sweep, made
    deterministic): small values, values next to p, every power of two and its
    negative, values next to 2^253, the halves and the third."""
    items = [(str(k), k) for k in range(1, 17)] + [("p-%d" % k, P - k) for k in range(1, 17)]
    for k in range(254):
        items.append(("2^%d" % k, 1 << k))
        items.append(("p-2^%d" % k, P - (1 << k)))
    items += [("2^253+2^%d" % k, (1 << 253) + (1 << k)) for k in range(30)]
    items += [("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2), ("p//3", P // 3)]
    assert all(0 < v < P for _, v in items)
    return _dedupe(items)


def field_values(items, views=VIEWS, field=O.FQ):
    """(label, v) pairs -> ("view label", field value) for each view of each v."""
    m = _MOD[field]
    un = _UNVIEW if field == O.FQ else _UNVIEW_R
    return [("%s %s" % (view, lab), v * un[view] % m) for view in views for lab, v in items]


def images(vals, field=O.FQ):
    """field values -> (n, 4) reference memory images."""
    return O.canon_to_mont_array(vals, field).reshape(-1, 4)


def fq_elements(views=VIEWS):
    """E0(p) in the given views: ((n, 4) images, labels, field values)."""
    fv = field_values(e0(P), views)
    vals = [v for _, v in fv]
    return images(vals), [lab for lab, _ in fv], vals


def filler(n, m=P, salt=0):
    g = O.SplitMix64(FILL_SEED + salt)
    return [g.below(m) for _ in range(n)]


# ---------------------------------------------------------------- Fq12 rows
def fq12_rows():
    """Structured Fq12 elements: ((n, 48) images, labels, rows of 12 field values).
    Coefficient order as the oracle's: index 6i + 2j + k."""
    rows = [("0", [0] * 12), ("1", [1] + [0] * 11), ("-1", [P - 1] + [0] * 11)]
    for c, name in ((1, "1"), (P - 1, "p-1")):
        for pos in range(12):
            rows.append(("%s at %d" % (name, pos), [c if i == pos else 0 for i in range(12)]))
    for lab, v in [("1", 1), ("2", 2), ("3", 3), ("p-1", P - 1), ("(p-1)/2", (P - 1) // 2), ("(p+1)/2", (P + 1) // 2)]:
        rows.append(("all = " + lab, [v] * 12))
    for lab, v in field_values(patterns(P), VIEWS):
        rows.append(("all = " + lab, [v] * 12))
    f = filler(12 * 16, salt=1)
    for k in range(4):
        r = f[48 * k:48 * k + 48]
        rows.append(("Fq only #%d" % k, r[:1] + [0] * 11))
        rows.append(("Fq2 only #%d" % k, r[12:14] + [0] * 10))
        rows.append(("Fq6 only #%d" % k, r[24:30] + [0] * 6))
        rows.append(("c0 = 0 #%d" % k, [0] * 6 + r[36:42]))
    f = filler(12 * 2, salt=2)
    for pos in (0, 11):
        for lab, v in field_values(e0(P), ("internal",)):
            r = f[:12] if pos == 0 else f[12:]
            rows.append(("%s at %d of random" % (lab, pos), [v if i == pos else r[i] for i in range(12)]))
    labels = [lab for lab, _ in rows]
    vals = [r for _, r in rows]
    arr = O.canon_to_mont_array([c for r in vals for c in r]).reshape(-1, 48)
    return arr, labels, vals


def fq12_subfield_mask(labels):
    """Rows of fq12_rows() that lie in Fq6 (c1 = 0) and are nonzero: their final
    exponentiation is exactly one ((p^6 - 1) kills Fq6*)."""
    def in_fq6(lab):
        if lab in ("1", "-1") or lab.startswith(("Fq only", "Fq2 only", "Fq6 only")):
            return True
        return " at " in lab and "random" not in lab and int(lab.split(" at ")[1]) < 6
    return np.array([in_fq6(lab) for lab in labels])


# ---------------------------------------------------------------- points
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


@functools.lru_cache(maxsize=None)
def g1_affine():
    """Structured affine G1 points, as (label, x, y) field values: both signs of y
    for every x in 0..39 and p-39..p-1 with x^3 + 3 a square (p = 3 mod 4), then
    k * G for k = 1..8.  G1 has cofactor 1: every one is a group element."""
    pts = []
    for x in list(range(40)) + [P - k for k in range(39, 0, -1)]:
        rhs = (x * x * x + 3) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            name = str(x) if x < 40 else "p-%d" % (P - x)
            pts.append(("x=%s +y" % name, x, y))
            pts.append(("x=%s -y" % name, x, P - y))
    k = O.canon_to_mont_array(range(1, 9), O.FR).reshape(8, 4)
    aff, rcs = O.g1_to_affine(O.g1_mul(O.g1_one(), k))
    assert rcs == [0] * 8
    for i in range(8):
        x, y = O.mont_array_to_canon(aff[i])
        pts.append(("%d*G" % (i + 1), x, y))
    return pts


@functools.lru_cache(maxsize=None)
def g2_affine():
    """k * G2 and (r - k) * G2 for k = 1..8, normalized: (label, (x0, x1), (y0, y1))."""
    ks = list(range(1, 9)) + [R - k for k in range(1, 9)]
    aff, rcs = O.g2_to_affine(O.g2_mul(O.g2_one(), O.canon_to_mont_array(ks, O.FR).reshape(16, 4)))
    assert rcs == [0] * 16
    pts = []
    for i, k in enumerate(ks):
        c = O.mont_array_to_canon(aff[i])
        pts.append((("%d*G2" % k) if k < 9 else "(r-%d)*G2" % (R - k), (c[0], c[1]), (c[2], c[3])))
    return pts


def g1_z_values():
    """Jacobian z for G1: E0(p) in all three views, zero excluded."""
    return [(lab, v) for lab, v in field_values(e0(P)) if v]


def g2_z_values(views=VIEWS):
    """Jacobian z for G2: (v, 0), (0, v), (v, v), (v, p - v) for v of g1_z_values()."""
    out = []
    for lab, v in field_values(e0(P), views):
        if v:
            out += [("(v,0) " + lab, (v, 0)), ("(0,v) " + lab, (0, v)), ("(v,v) " + lab, (v, v)),
                    ("(v,p-v) " + lab, (v, P - v))]
    return out


def g1_jacobian(pts, zs):
    """Row i: pts[i] rescaled to zs[i] -- (x z^2, y z^3, z).  (n, 12) images."""
    vals = []
    for (_, x, y), z in zip(pts, zs):
        vals += [x * z * z % P, y * z * z * z % P, z % P]
    return O.canon_to_mont_array(vals).reshape(-1, 12)


def g2_jacobian(pts, zs):
    """Row i: pts[i] rescaled to the Fq2 element zs[i].  (n, 24) images."""
    vals = []
    for (_, x, y), z in zip(pts, zs):
        z2 = _f2mul(z, z)
        vals += [*_f2mul(x, z2), *_f2mul(y, _f2mul(z2, z)), z[0] % P, z[1] % P]
    return O.canon_to_mont_array(vals).reshape(-1, 24)


def g1_affine_jac():
    """g1_affine() with z = one: ((n, 12) images, labels)."""
    pts = g1_affine()
    return g1_jacobian(pts, [1] * len(pts)), [p[0] for p in pts]


def g2_affine_jac():
    pts = g2_affine()
    return g2_jacobian(pts, [(1, 0)] * len(pts)), [p[0] for p in pts]


def g1_rescaled(shift=0):
    """Every structured G1 point and every z at least once: row i is point i mod nP
    at z (i + shift) mod nZ.  ((n, 12) rescaled, (n, 12) affine source, labels)."""
    pts, zs = g1_affine(), g1_z_values()
    n = max(len(pts), len(zs))
    src = [pts[i % len(pts)] for i in range(n)]
    z = [zs[(i + shift) % len(zs)] for i in range(n)]
    labels = ["%s, z: %s" % (s[0], zz[0]) for s, zz in zip(src, z)]
    return g1_jacobian(src, [v for _, v in z]), g1_jacobian(src, [1] * n), labels


def g2_rescaled(views=VIEWS, shift=0):
    pts, zs = g2_affine(), g2_z_values(views)
    n = max(len(pts), len(zs))
    src = [pts[i % len(pts)] for i in range(n)]
    z = [zs[(i + shift) % len(zs)] for i in range(n)]
    labels = ["%s, z: %s" % (s[0], zz[0]) for s, zz in zip(src, z)]
    return g2_jacobian(src, [v for _, v in z]), g2_jacobian(src, [(1, 0)] * n), labels


def gcd_points(point_index=3):
    """One fixed affine G1 point rescaled to z = u_g for every g of GCD(p), u_g the
    field value whose internal integer is g: ((n, 12) rescaled, (12,) source, labels)."""
    pt = g1_affine()[point_index]
    fv = field_values(gcd_sweep(), ("internal",))
    rescaled = g1_jacobian([pt] * len(fv), [v for _, v in fv])
    return rescaled, g1_jacobian([pt], [1])[0], ["z: " + lab for lab, _ in fv]


def zero_point(width):
    """(0, 1, 0): G1::zero() for width 12, G2::zero() for 24.  A zero z under other x, y is
    just as much a zero point to the reference (mod.rs:246-248), which defines the outcome
    of every operation on it; tests/group_exceptional_cases.py:zero_images generates those
    and tests/test_gpu_group_exceptional.py feeds them to every entry point."""
    z = np.zeros(width, np.uint64)
    z[width // 3:width // 3 + 4] = O.canon_to_mont_array([1]).reshape(4)
    return z


def pairing_pairs():
    """About 400 structured pairs: the rescaled structured G1 points against k * G2,
    then k * G against the rescaled G2 points (every internal-view z, a stride of the
    others).  ((n, 12) p, (n, 24) q, labels)."""
    p1, _, l1 = g1_rescaled()
    q_aff, ql = g2_affine_jac()
    n1 = 200
    pa = np.stack([p1[i % len(p1)] for i in range(n1)])
    qa = np.stack([q_aff[i % 16] for i in range(n1)])
    la = ["%s | %s" % (l1[i % len(l1)], ql[i % 16]) for i in range(n1)]
    q_int, _, li = g2_rescaled(("internal",))
    q_oth, _, lo = g2_rescaled(("field", "image"))
    pick = list(range(0, len(q_oth), 12))
    qb = np.concatenate([q_int, q_oth[pick]])
    lq = li + [lo[i] for i in pick]
    kg = g1_affine_jac()[0][-8:]
    pb = np.stack([kg[i % 8] for i in range(len(qb))])
    lb = ["%d*G | %s" % (i % 8 + 1, lab) for i, lab in enumerate(lq)]
    return np.concatenate([pa, pb]), np.concatenate([qa, qb]), la + lb


def one_product_terms(n):
    """n terms [(P_i, Q_i), (-P_i, Q_i), ...] of the structured pairs, whose pairing
    product is exactly one: 64 terms are 32 pairs spread over the set, other sizes
    the set from its start, tiled.  ((n, 12) p, (n, 24) q)."""
    p, q, _ = pairing_pairs()
    pn = np.empty((2 * p.shape[0], 12), np.uint64)
    pn[0::2], pn[1::2] = p, O.g1_neg(p)
    qn = np.repeat(q, 2, axis=0)
    if n == 64:
        idx = np.linspace(0, p.shape[0] - 1, 32).astype(int)
        idx = np.stack([2 * idx, 2 * idx + 1], axis=1).reshape(-1)
        return pn[idx], qn[idx]
    reps = n // len(pn) + 1
    return np.tile(pn, (reps, 1))[:n], np.tile(qn, (reps, 1))[:n]


# ---------------------------------------------------------------- scalars
def scalars():
    """E0(r) in the field-value and image views, the runs-of-ones and alternating
    patterns of test_gt_pow, r - 2^k: ((n, 4) Fr images, labels, canonical values)."""
    fv = field_values(e0(R), ("field", "image"), O.FR)
    fv += [("2^250-1", (1 << 250) - 1), ("2^253-1 run", (1 << 253) - 1), ("01*126", int("01" * 126, 2)),
           ("10000*50", int("10000" * 50, 2))]
    fv += [("r-2^%d" % k, R - (1 << k)) for k in (1, 64, 128, 253)]
    fv = _dedupe(fv)
    vals = [v for _, v in fv]
    return images(vals, O.FR), [lab for lab, _ in fv], vals


def cross(n_a, n_b, cap=2000):
    """Index pairs (i, j) of a strided cut through the n_a x n_b cross of at most
    about `cap` rows in which every i and every j occurs."""
    total = n_a * n_b
    stride = max(1, -(-total // cap))
    while np.gcd(stride, n_b) != 1:
        stride += 1
    assert stride < n_b
    idx = np.arange(0, total, stride)
    i, j = idx // n_b, idx % n_b  # (stride < n_b: every i; coprime to n_b: every j)
    assert set(i) == set(range(n_a)) and set(j) == set(range(n_b))
    return i, j


def digit_boundary_values():
    """Image-view integers next to every 29-bit digit boundary: 2^k - 1, 2^k, 2^k + 1
    for k = 29 i, and next to the 32- and 64-bit word boundaries, below p."""
    ks = sorted(set(range(29, 254, 29)) | set(range(32, 254, 32)))
    items = [(lab % k, f(1 << k)) for k in ks
             for lab, f in (("2^%d-1", lambda t: t - 1), ("2^%d", lambda t: t), ("2^%d+1", lambda t: t + 1))]
    return _dedupe([(lab, v) for lab, v in items if v < P])
