"""Inputs that drive the group law's exceptional branches (groups/mod.rs:246-350: self
zero, other zero, the doubling branch u1 == u2 && s1 == s2, and h == 0 with s1 != s2 whose
general formula gives z3 == 0) inside the scalar-multiplication and MSM kernels, shared by
tests/test_group_exceptional_cases.py (CPU) and tests/test_gpu_group_exceptional.py.

  * zero images: z == 0 under five different x, y;
  * twist points of order ELL = 10069 (the G2 twist has cofactor h2 = 2p - r, and ELL divides
    h2 exactly once): on the curve, so legal G2::new values, whose double-and-add chains walk
    through zero, res == Q and res == -Q at the bits chain_events() predicts from integers;
  * scalar families built to reach each of those events;
  * an affine integer model of the twist (chord and tangent, explicit infinity), a second
    witness that shares no formula with the oracle's Jacobian law;
  * MSM families over the bases j * G, j in +-{1..4}, where nearly every bucket sum, running
    sum and window combination meets an equal or an opposite point; the expected row comes
    from the integer sum of k_i * j_i, not from a tree of additions.

Oracle plus Python integers; no GPU import."""
import functools

import numpy as np

from oracle import oracle as O
from tests import edge_vectors as EV

P, R = O.P, O.R
ELL = 10069
H2 = 2 * P - R            # cofactor of the twist: #E'(Fq2) = H2 * R
COFACTOR = H2 // ELL      # 241 bits: a valid Fr value
SEED = 0x6C0FAC70
WIDTH = {"g1": 12, "g2": 24}
SMALL_JS = (1, 2, 3, 4, -1, -2, -3, -4)
KINDS = ("cancel", "same", "zero_plus", "double_of_zero")

assert H2 % ELL == 0 and COFACTOR % ELL != 0 and COFACTOR < R and COFACTOR.bit_length() == 241
assert H2 == 10069 * 5864401 * 1875725156269 * 197620364512881247228717050342013327560683201906968909

_MUL = {"g1": O.g1_mul, "g2": O.g2_mul}
_ADD = {"g1": O.g1_add, "g2": O.g2_add}
_NEG = {"g1": O.g1_neg, "g2": O.g2_neg}
_NORM = {"g1": O.g1_normalize, "g2": O.g2_normalize}
_ONE = {"g1": O.g1_one, "g2": O.g2_one}


def fr(vals):
    """canonical integers -> (n, 4) Montgomery Fr images"""
    return O.canon_to_mont_array([int(v) % R for v in vals], O.FR).reshape(len(vals), 4)


def zero(group):
    """(0, one, 0)"""
    return EV.zero_point(WIDTH[group])


def is_zero(img):
    """z == 0, for one image or for rows of images"""
    img = np.asarray(img)
    return ~img[..., 2 * img.shape[-1] // 3:].any(axis=-1)


# ---------------------------------------------------------------- Fq2 and Jacobian rescaling, integers
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def rescale(img, lam):
    """The same point in another Jacobian scaling: (x lam^2, y lam^3, z lam).  img: one G1 or
    G2 image; lam: an integer (G1) or a pair (G2), nonzero."""
    c = O.mont_array_to_canon(img)
    if len(c) == 3:
        x, y, z = c
        out = [x * lam * lam % P, y * lam * lam * lam % P, z * lam % P]
    else:
        x, y, z = (c[0], c[1]), (c[2], c[3]), (c[4], c[5])
        l2 = _f2mul(lam, lam)
        out = [*_f2mul(x, l2), *_f2mul(y, _f2mul(l2, lam)), *_f2mul(z, lam)]
    return O.canon_to_mont_array(out)


def _lams(group, n, salt):
    g = O.SplitMix64(SEED + salt)
    if group == "g1":
        return [2 + g.below(P - 2) for _ in range(n)]
    return [(2 + g.below(P - 2), 1 + g.below(P - 1)) for _ in range(n)]


# ---------------------------------------------------------------- zero images
@functools.lru_cache(maxsize=None)
def _zero_images(group):
    w = WIDTH[group]
    t = w // 3
    g3 = _NORM[group](_MUL[group](_ONE[group](), fr([3])))[0]
    on_curve = g3.copy()
    on_curve[2 * t:] = 0
    p = _MUL[group](_ONE[group](), fr([0x1F2E3D4C5B6A7988]))
    natural = _ADD[group](p, _NEG[group](p))[0]
    assert is_zero(natural) and natural[:2 * t].any()
    un = pow(1 << 261, -1, P)
    a, b = (P - 1) * un % P, ((1 << 232) - 1) * un % P   # internal integers p - 1 and 2^232 - 1 (fq.h: R = 2^261)
    assert ("internal p-1", a) in EV.field_values(EV.e0(P), ("internal",))
    assert ("internal 2^232-1", b) in EV.field_values(EV.e0(P), ("internal",))
    xy = [a, b, 0] if group == "g1" else [a, b, b, a, 0, 0]
    rows = [("(0, one, 0)", zero(group)),
            ("on-curve x, y of 3G, z = 0", on_curve),
            ("P - P by the oracle", natural),
            ("(0, 0, 0)", np.zeros(w, np.uint64)),
            ("internal p-1, 2^232-1, z = 0", O.canon_to_mont_array(xy))]
    arr = np.stack([r for _, r in rows])
    arr.setflags(write=False)
    return arr, tuple(lab for lab, _ in rows)


def zero_images(group):
    """Five images with z == 0: ((5, width) images, labels)."""
    arr, labels = _zero_images(group)
    return arr.copy(), list(labels)


# ---------------------------------------------------------------- the affine integer model of the twist
@functools.lru_cache(maxsize=None)
def twist_b():
    """b' of the twist from the generator: y^2 - x^3 (groups/mod.rs:452-467)"""
    c = O.mont_array_to_canon(O.g2_one())
    x, y = (c[0], c[1]), (c[2], c[3])
    y2, x3 = _f2mul(y, y), _f2mul(_f2mul(x, x), x)
    return ((y2[0] - x3[0]) % P, (y2[1] - x3[1]) % P)


def random_twist_points(n, seed):
    """(x, y) on E'(Fq2) but (almost surely) outside the order-r subgroup: (n, 8) images each."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    b = twist_b()
    while len(xs) < n:
        x = O.canon_to_mont_array([int.from_bytes(rng.bytes(32), "big") % P for _ in range(2)])
        x3 = O.binary("orc_fq2_mul", O.binary("orc_fq2_mul", x, x, 8, 8, 8), x, 8, 8, 8)
        rhs = [(u + v) % P for u, v in zip(O.mont_array_to_canon(x3), b)]
        y, ok = O.fq2_sqrt(O.canon_to_mont_array(rhs))
        if ok[0]:
            xs.append(x.reshape(8))
            ys.append(y.reshape(8))
    return np.stack(xs), np.stack(ys)


def model_on_curve(a):
    if a is None:
        return True
    x, y = a
    y2, x3, b = _f2mul(y, y), _f2mul(_f2mul(x, x), x), twist_b()
    return y2 == ((x3[0] + b[0]) % P, (x3[1] + b[1]) % P)


def model_add(a, b):
    """chord and tangent on y^2 = x^3 + b' over Fq2; None is the point at infinity"""
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if ((y1[0] + y2[0]) % P, (y1[1] + y2[1]) % P) == (0, 0):
            return None
        xx = _f2mul(x1, x1)
        lam = _f2mul((3 * xx[0] % P, 3 * xx[1] % P), _f2inv((2 * y1[0] % P, 2 * y1[1] % P)))
    else:
        lam = _f2mul(((y2[0] - y1[0]) % P, (y2[1] - y1[1]) % P), _f2inv(((x2[0] - x1[0]) % P, (x2[1] - x1[1]) % P)))
    l2 = _f2mul(lam, lam)
    x3 = ((l2[0] - x1[0] - x2[0]) % P, (l2[1] - x1[1] - x2[1]) % P)
    t = _f2mul(lam, ((x1[0] - x3[0]) % P, (x1[1] - x3[1]) % P))
    return (x3, ((t[0] - y1[0]) % P, (t[1] - y1[1]) % P))


def model_mul(k, a):
    acc = None
    while k:
        if k & 1:
            acc = model_add(acc, a)
        a = model_add(a, a)
        k >>= 1
    return acc


def model_point(img):
    """a G2 image as the model's affine point; None when z == 0"""
    c = O.mont_array_to_canon(img)
    z = (c[4], c[5])
    if z == (0, 0):
        return None
    zi = _f2inv(z)
    zi2 = _f2mul(zi, zi)
    return (_f2mul((c[0], c[1]), zi2), _f2mul((c[2], c[3]), _f2mul(zi2, zi)))


# ---------------------------------------------------------------- twist points of order ELL
@functools.lru_cache(maxsize=None)
def _order_ell_base():
    one = np.zeros(8, np.uint64)
    one[:4] = O.canon_to_mont_array([1]).reshape(4)
    for seed in range(11, 43):
        x, y = random_twist_points(1, seed)
        t = np.concatenate([x[0], y[0], one])
        ct = O.g2_mul(t, fr([COFACTOR]))
        q = O.g2_add(O.g2_mul(ct, fr([R - 1])), ct)[0]          # r * (c * T): order divides ELL
        if is_zero(q):
            continue
        assert is_zero(O.g2_mul(q, fr([ELL]))[0])
        q.setflags(write=False)
        return q
    raise AssertionError("no twist point of order %d in 32 draws" % ELL)


def order_ell_q():
    """Q of order ELL on the twist, as the oracle's Jacobian image (z != one)."""
    return _order_ell_base().copy()


ELL_JS = (1, 2, 3, 5, 7, 100, (ELL - 1) // 2, (ELL + 1) // 2, ELL - 2, ELL - 1)


@functools.lru_cache(maxsize=None)
def _order_ell_points():
    q = _order_ell_base()
    imgs = O.g2_mul(q, fr(ELL_JS))          # j < ELL: no prefix of the chain is 0 or -1 mod ELL before an add
    lams = _lams("g2", len(ELL_JS), 1)
    rows, labels, js = [], [], []
    for i, j in enumerate(ELL_JS):
        rows += [imgs[i], rescale(imgs[i], lams[i])]
        labels += ["%d*Q" % j, "%d*Q rescaled" % j]
        js += [j, j]
    arr = np.stack(rows)
    arr.setflags(write=False)
    return arr, tuple(labels), tuple(js)


def order_ell_points():
    """Q and several j * Q, each in two Jacobian scalings: ((n, 24) images, labels, the j)."""
    arr, labels, js = _order_ell_points()
    return arr.copy(), list(labels), list(js)


def chain_events(k, ell=ELL):
    """The exceptional steps of the reference's chain for k * Q (mod.rs:275-292), Q of odd
    order ell, from integers alone: the bits of k from the top, the prefix m mod ell.
    Returns [(bit, kind)]:
      "double_of_zero"  a doubling of res == zero (m == 0);
      "cancel"          an addition res + Q with res == -Q (m doubled to -1);
      "same"            an addition with res == Q (m doubled to 1): the doubling branch;
      "zero_plus"       an addition onto res == zero after the chain's first one."""
    events = []
    m, found = 0, False
    for bit in range(255, -1, -1):
        if found:
            if m == 0:
                events.append((bit, "double_of_zero"))
            m = 2 * m % ell
        if (k >> bit) & 1:
            if found:
                if m == 0:
                    events.append((bit, "zero_plus"))
                elif m == ell - 1:
                    events.append((bit, "cancel"))
                elif m == 1:
                    events.append((bit, "same"))
            found = True
            m = (m + 1) % ell
    assert m == k % ell
    return events


def event_kinds(k, ell=ELL):
    return {kind for _, kind in chain_events(k, ell)}


def _extend(k, t, g):
    """k followed by t random low bits"""
    return (k << t) | g.below(1 << t)


@functools.lru_cache(maxsize=None)
def order_ell_scalars():
    """{family: [(label, k)]} for points of order ELL, every k below r:
      "same"      ELL + 2 and extensions: the prefix (ELL + 1) / 2 doubles to 1 under a set bit;
      "cancel"    ELL * 2^s + b, 0 < b < 2^s, and extensions: cancel, then s doublings of a
                  zero image, then zero_plus;
      "multiple"  multiples of ELL: the result is a zero image;
      "uniform"   256 uniform scalars (about 7 % meet an event by chance)."""
    g = O.SplitMix64(SEED + 2)
    fam = {"same": [("ELL+2", ELL + 2)], "cancel": [], "multiple": [], "uniform": []}
    for t in (1, 5, 64, 200, 239):
        fam["same"].append(("(ELL+2) then %d bits" % t, _extend(ELL + 2, t, g)))
    for s, b in ((1, 1), (2, 1), (3, 5), (7, 64), (30, (1 << 30) - 1), (100, 1 + (1 << 99))):
        k = (ELL << s) + b
        fam["cancel"].append(("ELL*2^%d+%d" % (s, b), k))
        for t in (3, 130):
            fam["cancel"].append(("(ELL*2^%d+%d) then %d bits" % (s, b, t), _extend(k, t, g)))
    fam["multiple"] = [("ELL", ELL), ("2*ELL", 2 * ELL), ("ELL*2^200", ELL << 200), ("ELL*ELL", ELL * ELL)]
    for i in range(12):
        v = g.below(R // ELL)
        fam["multiple"].append(("ELL*random #%d" % i, ELL * v))
    fam["multiple"].append(("ELL*(r//ELL)", ELL * (R // ELL)))
    fam["uniform"] = [("uniform #%d" % i, g.below(R)) for i in range(256)]
    assert all(0 < k < R for rows in fam.values() for _, k in rows)
    return fam


def event_counts():
    """{family: {kind: rows of the family whose chain meets it}}"""
    return {name: {kind: sum(kind in event_kinds(k) for _, k in rows) for kind in KINDS}
            for name, rows in order_ell_scalars().items()}


def zero_image_scalars():
    """Scalars for k * (a zero image): the result is double^t of the image, t the number of
    trailing zero bits of k (every addition returns the base, mod.rs:298-300).  (label, k)."""
    g = O.SplitMix64(SEED + 3)
    rows = [(str(k), k) for k in (0, 1, 2, 3, 4)]
    for e in (5, 31, 32, 64, 128, 253):
        rows += [("2^%d" % e, 1 << e), ("2^%d+1" % e, (1 << e) + 1)]
    rows.append(("r-1", R - 1))
    for t in range(6):
        for i in range(3):
            v = (g.below(R >> (t + 1)) << (t + 1)) | (1 << t)
            rows.append(("random, %d trailing zeros #%d" % (t, i), v))
    assert all(0 <= k < R for _, k in rows)
    return rows


def trailing_zeros(k):
    return (k & -k).bit_length() - 1 if k else 0


# ---------------------------------------------------------------- dense-collision MSM families
@functools.lru_cache(maxsize=None)
def _small_multiples(group):
    """{j: the normalized image of j * G} for j in SMALL_JS"""
    imgs = _NORM[group](_MUL[group](_ONE[group](), fr(SMALL_JS)))
    imgs.setflags(write=False)
    return {j: imgs[i] for i, j in enumerate(SMALL_JS)}


def small_multiple_points(group, js, salt=0):
    """Row i: js[i] * G, rescaled to a random z != one except every fourth row, left at
    z == one; js[i] == 0 gives a zero image, the five of zero_images() in turn."""
    base = _small_multiples(group)
    zs, _ = _zero_images(group)
    lams = _lams(group, len(js), 16 + salt)
    rows, nz = [], 0
    for i, j in enumerate(js):
        if j == 0:
            rows.append(zs[nz % len(zs)])
            nz += 1
        elif i % 4 == 3:
            rows.append(base[j])
        else:
            rows.append(rescale(base[j], lams[i]))
    return np.stack(rows) if rows else np.zeros((0, WIDTH[group]), np.uint64)


def expected_sum(group, js, ks):
    """normalize(G * (sum k_i j_i mod r)), or (0, one, 0) when the sum is 0 mod r"""
    s = sum(int(k) * int(j) for j, k in zip(js, ks)) % R
    if s == 0:
        return zero(group)
    return _NORM[group](_MUL[group](_ONE[group](), fr([s])))[0]


def every_bucket_equal(c, alternating=False):
    """For window width c and every window w, one term (G, d * 2^(c w)) per digit
    d = 1 .. 2^(c-1): every bucket of every window holds exactly G, so the running sums are
    G + G, then 3G + 3G, ...  With `alternating` the bases are G, -G, G, ...: the running sums
    cancel to zero images and restart.  (js, ks)."""
    js, ks = [], []
    for w in range(254 // c + 1):
        for d in range(1, (1 << (c - 1)) + 1):
            k = d << (c * w)
            if k < R:
                js.append(-1 if alternating and len(js) % 2 else 1)
                ks.append(k)
    return js, ks


def random_small_multiples(n=1024, salt=0, total_cancels=False, zeros=0):
    """n terms, j uniform in +-{1..4}, uniform 254-bit scalars; `zeros` further terms whose
    base is a zero image; with total_cancels one more term that makes the sum 0 mod r."""
    g = O.SplitMix64(SEED + 32 + salt)
    js = [SMALL_JS[g.below(8)] for _ in range(n)] + [0] * zeros
    ks = [g.below(R) for _ in range(n + zeros)]
    if total_cancels:
        s = sum(k * j for j, k in zip(js, ks)) % R
        js.append(1)
        ks.append((R - s) % R)
    return js, ks


def dense_families(group):
    """[(name, (n, width) points, canonical scalars, expected row)]"""
    fams = [("every bucket equal, c=5", every_bucket_equal(5)),
            ("every bucket equal, c=2", every_bucket_equal(2)),
            ("alternating, c=5", every_bucket_equal(5, True)),
            ("alternating, c=2", every_bucket_equal(2, True)),
            ("random small multiples", random_small_multiples(1024, 0, zeros=5)),
            ("total cancels", random_small_multiples(1024, 0, True, zeros=5))]
    out = []
    for i, (name, (js, ks)) in enumerate(fams):
        out.append((name, small_multiple_points(group, js, i), ks, expected_sum(group, js, ks)))
    return out


def many_segments(unit):
    """The dense families cut for bn_g1_msm_many: segments of 1, 2, T, T + 1 and 3T terms
    (T = unit) in turn over the every-bucket-equal (c = 4), alternating and random terms, and
    one segment whose sum cancels.  (points, canonical scalars, offsets, expected rows)."""
    js, ks = [], []
    for part in (every_bucket_equal(4), every_bucket_equal(4, True), random_small_multiples(256, 5, zeros=5)):
        js += part[0]
        ks += part[1]
    lens, n = [], 0
    while n < len(js):
        for length in (1, 2, unit, unit + 1, 3 * unit):
            length = min(length, len(js) - n)
            if length:
                lens.append(length)
                n += length
    cj, ck = random_small_multiples(3 * unit, 6, True)
    js, ks, lens = js + cj, ks + ck, lens + [len(cj)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uintp)
    want = np.stack([expected_sum("g1", js[int(a):int(b)], ks[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])])
    assert np.array_equal(want[-1], zero("g1"))
    return small_multiple_points("g1", js, 40 + unit), ks, off, want


PREPARED_JS = (1, 1, -1, 2, -2, 1, 0)


def prepared_case(c):
    """bn_g1_msm_prepared_many over the bases [G, G in another scaling, -G, 2G, -2G, G, a zero
    image] with rows of small, equal and full-width scalars (and the digit boundaries of
    width c).  (bases, (m, 7) canonical scalars, expected rows)."""
    js = list(PREPARED_JS)
    bases = small_multiple_points("g1", js, 60)
    bases[0] = _small_multiples("g1")[1]          # G at z == one beside G rescaled
    g = O.SplitMix64(SEED + 64 + c)
    rows = [[0] * 7, [1] * 7, [1, 1, 0, 0, 0, 0, 5], [1, 0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 1, 0, 0], [2, 0, 0, 0, 1, 0, 0],
            [1, 1, 0, 1, 0, 1, 0], [3, 2, 1, 1, 2, 3, 9], [R - 1] * 7, [R - 1, 1, 0, 0, 0, 0, 0]]
    for w in (1, (254 // c + 1) // 2, 254 // c):
        for v in ((1 << (c * w)) % R, ((1 << (c * w)) - 1) % R, (1 << (c * w - 1)) % R):
            rows += [[v] * 7, [v, v, v, 0, 0, 0, 1], [v, 0, 0, v, v, v, 0]]
    for _ in range(8):
        v = g.below(R)
        rows += [[v] * 7, [v, R - v, 0, v, v, 0, v]]
    rows += [[g.below(1 << 8) for _ in range(7)] for _ in range(8)]
    rows += [[g.below(R) for _ in range(7)] for _ in range(16)]
    want = np.stack([expected_sum("g1", js, row) for row in rows])
    return bases, rows, want


def order_ell_msm(n=512):
    """A G2 MSM that lives in a group of ELL elements: bases j_i * Q (both scalings), uniform
    254-bit scalars; collisions at nearly every reduction step.  (points, canonical scalars,
    expected row, s = sum k_i j_i mod ELL)."""
    pts, _, js_all = order_ell_points()
    g = O.SplitMix64(SEED + 96)
    idx = [g.below(len(js_all)) for _ in range(n)]
    ks = [g.below(R) for _ in range(n)]
    s = sum(k * js_all[i] for i, k in zip(idx, ks)) % ELL
    if s == 0:
        ks[0] = (ks[0] + 1) % R
        s = js_all[idx[0]] % ELL
    want = O.g2_normalize(O.g2_mul(order_ell_q(), fr([s])))[0]
    return pts[idx], ks, want, s
