"""Edge-operand parity of the MI355X kernels (through the C ABI) with the oracle,
bit for bit: the structured vectors of tests/edge_vectors.py -- field elements,
Jacobian z and scalars on the digit, carry, fold and zero boundaries, in the
field-value, memory-image and internal-integer views -- through the field,
group, pairing, final-exponentiation, Gt::pow and codec kernels on every path.
Every vector is compared; a failure names the vector.  The CPU half
(tests/test_edge_vectors.py) pins the oracle on the same vectors.
Runs on the GPU box: python -m pytest tests -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_vectors as E
from tests.codec_util import be, compress_g1, compress_g2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
NT = 16
P, R = O.P, O.R
ONE12 = O.canon_to_mont_array([1] + [0] * 11)


def same(got, want, labels, what):
    """np.array_equal with the failing vectors named."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.shape[0] == len(labels), (what, got.shape, want.shape, len(labels))
    bad = np.flatnonzero((got != want).reshape(len(labels), -1).any(axis=1))
    assert bad.size == 0, "%s: %d of %d rows differ, first: %s" % (what, bad.size, len(labels),
                                                                  [labels[i] for i in bad[:5]])
    assert np.array_equal(got, want)


def _threaded(fn, n):
    """fn(rows) over NT slices of range(n) on host threads (the oracle's C calls
    release the GIL): the per-slice results, in order."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(NT) as ex:
        return list(ex.map(fn, [c for c in np.array_split(np.arange(n), NT) if len(c)]))


def oracle_gt_pow(a, k):
    return np.concatenate(_threaded(lambda c: O.gt_pow(a[c], k[c]), a.shape[0]))


def oracle_miller_product(q, p):
    """O.miller_loop_batch(q, p): the shared loop's value is the product of the
    terms' Miller values, an exact field identity, so slices are multiplied up."""
    parts = _threaded(lambda c: O.miller_loop_batch(q[c], p[c]), q.shape[0])
    assert all(rc == 0 for rc, _ in parts)
    f = parts[0][1]
    for _, g in parts[1:]:
        f = O.binary("orc_fq12_mul", f, g, 48, 48, 48)[0]
    return f


def _ctx(fe_wide_max=None, latency_max=None):
    from substrate_bn import Context
    c = Context(0)
    if fe_wide_max is not None:
        c.set_fe_wide_max(fe_wide_max)
    if latency_max is not None:
        c.set_latency_max(latency_max)
    return c


@pytest.fixture(scope="module")
def ctx():
    """Default thresholds: small pairing_many batches run k_pairing_latency."""
    return _ctx()


@pytest.fixture(scope="module")
def ctx_tp():
    """Every pairing_many batch on the throughput path (k_pairing_full)."""
    return _ctx(fe_wide_max=0)


@pytest.fixture(scope="module")
def ctx_seg():
    """Small batches on the segmented latency path (k_prepare_wide + k_miller_seg)."""
    return _ctx(latency_max=0)


@pytest.fixture(scope="module")
def ctx_w2():
    """Above 2,048 pairs the one-launch path runs the two-wave build."""
    return _ctx(latency_max=4096)


@pytest.fixture(scope="module")
def fq12():
    return E.fq12_rows()


@pytest.fixture(scope="module")
def pp():
    """The structured pairs and the oracle's Gt of each, computed once."""
    p, q, labels = E.pairing_pairs()
    return p, q, labels, O.pairing_many(p, q, NT)


def _frob(a, pw):
    want = np.zeros_like(a)
    for k in range(a.shape[0]):
        O.lib().orc_fq12_frobenius_map(O._p(a[k]), pw, O._p(want[k]))
    return want


# ---------------------------------------------------------------- 1. Fq12 operations
def test_fq12_ops_on_structured_rows(ctx, fq12):
    """All eight fq12_op_many ops on the structured rows; mul against a rotated copy
    of the set (structured times structured); zero through inv gives zero."""
    a, labels, _ = fq12
    b = np.roll(a, -1, axis=0)
    same(ctx.fq12_op_many("mul", a, b), O.binary("orc_fq12_mul", a, b, 48, 48, 48), labels, "mul")
    same(ctx.fq12_op_many("mul", a, a), O.binary("orc_fq12_mul", a, a, 48, 48, 48), labels, "mul a*a")
    same(ctx.fq12_op_many("sqr", a), O.unary("orc_fq12_squared", a, 48)[0], labels, "sqr")
    inv = ctx.fq12_op_many("inv", a)
    same(inv, O.unary("orc_fq12_inverse", a, 48)[0], labels, "inv")
    assert labels[0] == "0" and not inv[0].any()
    same(ctx.fq12_op_many("cyc_sqr", a), O.unary("orc_fq12_cyclotomic_squared", a, 48)[0], labels, "cyc_sqr")
    same(ctx.fq12_op_many("exp_by_neg_z", a), O.unary("orc_fq12_exp_by_neg_z", a, 48)[0], labels, "exp_by_neg_z")
    for pw in (1, 2, 3):
        same(ctx.fq12_op_many("frob%d" % pw, a), _frob(a, pw), labels, "frob%d" % pw)


# ---------------------------------------------------------------- 2. the inversion sweep, pairing paths
@pytest.fixture(scope="module")
def gcd():
    """One G1 point at z = u_g for every g of GCD(p), against one affine G2 point
    (N(qz) = 1): the operand of the pairing's to_affine inversion is exactly g."""
    resc, src, labels = E.gcd_points()
    q = np.tile(E.g2_affine_jac()[0][2], (resc.shape[0], 1))
    want = O.pairing_many(resc, q, NT)
    return resc, src, q, labels, want


@pytest.mark.parametrize("path", ["latency", "segmented", "throughput"])
def test_inversion_sweep_through_pairing(ctx, ctx_seg, ctx_tp, gcd, path):
    """latency: k_pairing_latency (fq_inv_quad in the producer); segmented:
    k_prepare_wide (fq_inv_quad on eight lanes); throughput: k_pairing_full
    (fq_inv_bgcd with the LDS fold).  Every row is the same point in another
    scaling, so every Gt must also equal row 0's: a failure of that alone is in the
    conversion, not in the Miller loop."""
    c = {"latency": ctx, "segmented": ctx_seg, "throughput": ctx_tp}[path]
    resc, src, q, labels, want = gcd
    assert len(labels) >= 550
    got = c.pairing_many(resc, q)
    same(got, np.tile(got[0], (len(labels), 1)), labels, path + ": row == row 0")
    same(got, want, labels, path)
    # waves that mix the z == one shortcut with the inversion, then 128 rows that all
    # take the shortcut, then inversions again
    n = len(labels)
    m = 2 * n + 128 + 64
    p2 = np.empty((m, 12), np.uint64)
    p2[0:2 * n:2], p2[1:2 * n:2], p2[2 * n:2 * n + 128], p2[2 * n + 128:] = resc, src, src, resc[:64]
    want2 = np.empty((m, 48), np.uint64)
    want2[:] = O.pairing_many(src, q[:1])[0]
    want2[0:2 * n:2], want2[2 * n + 128:] = want, want[:64]
    lab2 = [x for lab in labels for x in (lab, "z = one after " + lab)] + ["z = one"] * 128 + labels[:64]
    same(c.pairing_many(p2, np.tile(q[0], (m, 1))), want2, lab2, path + " interleaved with z = one")


# ---------------------------------------------------------------- 3. the sweep through normalize and eq
def test_inversion_sweep_through_normalize(ctx, gcd):
    """group_op_many normalize runs the device fq_inv_bgcd on z: G1 at every g of
    GCD(p), G2 at the whole G2 z set; eq with the affine source is 1, with its
    negation 0."""
    resc, src, _, labels, _ = gcd
    n = len(labels)
    srcs = np.tile(src, (n, 1))
    same(ctx.group_op_many("g1", "normalize", resc), srcs, labels, "g1 normalize == source")
    same(ctx.group_op_many("g1", "normalize", resc), O.g1_normalize(resc), labels, "g1 normalize")
    assert ctx.group_op_many("g1", "eq", resc, srcs).all()
    assert not ctx.group_op_many("g1", "eq", resc, O.g1_neg(srcs)).any()
    assert not ctx.group_op_many("g1", "eq", O.g1_neg(resc), srcs).any()
    r2, s2, l2 = E.g2_rescaled()
    assert len(l2) >= 480
    same(ctx.group_op_many("g2", "normalize", r2), s2, l2, "g2 normalize == source")
    same(ctx.group_op_many("g2", "normalize", r2), O.g2_normalize(r2), l2, "g2 normalize")
    same(ctx.group_op_many("g2", "eq", r2, s2)[:, None], np.ones((len(l2), 1), np.uint8), l2, "g2 eq source")
    same(ctx.group_op_many("g2", "eq", r2, O.g2_neg(s2))[:, None], np.zeros((len(l2), 1), np.uint8), l2, "g2 eq -source")
    r1, s1, l1 = E.g1_rescaled()
    same(ctx.group_op_many("g1", "normalize", r1), s1, l1, "g1 normalize, E0 z")
    same(ctx.group_op_many("g1", "eq", r1, s1)[:, None], np.ones((len(l1), 1), np.uint8), l1, "g1 eq source")
    same(ctx.group_op_many("g1", "eq", r1, O.g1_neg(s1))[:, None], np.zeros((len(l1), 1), np.uint8), l1, "g1 eq -source")


# ---------------------------------------------------------------- 4. group law
ORACLE = {
    "g1": {"add": O.g1_add, "sub": O.g1_sub, "neg": O.g1_neg, "eq": O.g1_eq},
    "g2": {"add": O.g2_add, "sub": O.g2_sub, "neg": O.g2_neg, "eq": O.g2_eq},
}


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_group_law_on_structured_points(ctx, group):
    """add, sub, neg, eq: every structured point, affine and rescaled, with itself,
    itself in another scaling, its negation, its negation in another scaling, and
    the next point of the set; at 1, 63 and all rows."""
    resc_fn = E.g1_rescaled if group == "g1" else E.g2_rescaled
    r0, src, l0 = resc_fn()
    r1 = resc_fn(shift=17)[0]
    neg = ORACLE[group]["neg"]
    a = np.concatenate([src, r0])
    la = ["affine " + x for x in l0] + l0
    others = {
        "itself": a,
        "itself rescaled": np.concatenate([r0, r1]),
        "negation": neg(a),
        "negation rescaled": neg(np.concatenate([r0, r1])),
        "next point": np.roll(a, -1, axis=0),
        "the zero point": np.tile(E.zero_point(a.shape[1]), (a.shape[0], 1)),  # (0, 1, 0), as tests/test_gpu_group.py
    }
    full = a.shape[0]
    for n in (1, 63, full):
        same(ctx.group_op_many(group, "neg", a[:n]), neg(a[:n]), la[:n], "%s neg n=%d" % (group, n))
        for name, b in others.items():
            for op in ("add", "sub"):
                same(ctx.group_op_many(group, op, a[:n], b[:n]), ORACLE[group][op](a[:n], b[:n]), la[:n],
                     "%s %s with %s n=%d" % (group, op, name, n))
            want = np.array(ORACLE[group]["eq"](a[:n], b[:n]), np.uint8)
            same(ctx.group_op_many(group, "eq", a[:n], b[:n])[:, None], want[:, None], la[:n],
                 "%s eq with %s n=%d" % (group, name, n))
            if name.startswith("itself"):
                assert want.all()
            if name.startswith("negation"):
                assert not want.any()


# ---------------------------------------------------------------- 5. scalar multiplication
def _mul_cross(group):
    k, kl, _ = E.scalars()
    if group == "g1":
        r, src, lab = E.g1_rescaled()
        aff, al = E.g1_affine_jac()
    else:
        r, src, lab = E.g2_rescaled()  # z in all three views, all four shapes
        aff, al = E.g2_affine_jac()
    pts = np.concatenate([aff, r, E.zero_point(aff.shape[1])[None, :]])  # (0, 1, 0), as test_g1_mul's edge rows
    pl = ["affine " + x for x in al] + lab + ["the zero point"]
    i, j = E.cross(len(pl), len(kl))
    assert set(i) == set(range(len(pl))) and set(j) == set(range(len(kl)))  # every point, every scalar
    assert 1000 <= len(i) <= 2000
    return pts[i], k[j], ["%s * %s" % (kl[b], pl[a]) for a, b in zip(i, j)]


def test_g1_mul_on_structured_points(ctx):
    """Structured points and rescalings crossed with the scalar set, raw Jacobian
    image: once as an odd batch of its own size (k_g1_mul), once planted in an odd
    batch past 2^18 of filler rows, at rows 0.., h.. and the tail (h = ceil(n / 2)),
    so that both chains of a lane of k_g1_mul2 and the lone last chain hold
    structured rows."""
    pts, k, labels = _mul_cross("g1")
    filler_p = O.g1_mul(O.g1_one(), O.canon_to_mont_array(E.filler(7, R, salt=5), O.FR).reshape(7, 4))
    filler_k = O.canon_to_mont_array(E.filler(11, R, salt=6), O.FR).reshape(11, 4)
    if len(labels) % 2 == 0:  # a filler row at index 1 makes the size odd
        pts, k = np.insert(pts, 1, filler_p[0], axis=0), np.insert(k, 1, filler_k[0], axis=0)
        labels = labels[:1] + ["filler"] + labels[1:]
    m = len(labels)
    assert m % 2 == 1 and m > 64
    want = O.g1_mul(pts, k, NT)
    same(ctx.g1_mul_many(pts, k), want, labels, "g1_mul")
    n = (1 << 18) + 1
    h = (n + 1) // 2
    big_p = np.tile(filler_p, (n // 7 + 1, 1))[:n].copy()
    big_k = np.tile(filler_k, (n // 11 + 1, 1))[:n].copy()
    t = m // 3
    rows = np.r_[0:t, h - 1:h - 1 + t, n - (m - 2 * t):n]  # lane h - 1 holds the lone chain (row h - 1)
    assert len(rows) == m and len(set(rows)) == m
    big_p[rows], big_k[rows] = pts, k
    same(ctx.g1_mul_many(big_p, big_k)[rows], want, labels, "g1_mul planted in 2^18 + 1")


def test_g2_mul_on_structured_points(ctx):
    """k * G2, (r - k) * G2 and every G2 rescaling (z of the four shapes, in all three
    views) crossed with the scalar set on k_g2_mul_split, raw Jacobian image."""
    pts, k, labels = _mul_cross("g2")
    assert len({lab.split(" * ", 1)[1] for lab in labels}) >= 16 + 480 + 1
    same(ctx.g2_mul_many(pts, k), O.g2_mul(pts, k, NT), labels, "g2_mul")


# ---------------------------------------------------------------- 6. pairing, Miller loop, line coefficients
@pytest.mark.parametrize("path", ["latency", "segmented", "throughput", "form0", "form1", "form2", "two_wave"])
def test_pairing_on_structured_pairs(ctx, ctx_seg, ctx_tp, ctx_w2, pp, path, monkeypatch):
    """pairing_many of the structured pairs on the three contexts of the inversion
    sweep, the A/B forms of the throughput path (BN254MI_MILLER_FORM 0, 1, 2), and
    the two-wave latency kernel with the set tiled to 2,049 rows."""
    p, q, labels, want = pp
    assert len(labels) >= 380
    if path.startswith("form"):
        monkeypatch.setenv("BN254MI_MILLER_FORM", path[4:])
        c = _ctx(fe_wide_max=0)
    else:
        c = {"latency": ctx, "segmented": ctx_seg, "throughput": ctx_tp, "two_wave": ctx_w2}[path]
    if path == "two_wave":
        reps = 2049 // len(labels) + 1
        p, q, want = (np.tile(x, (reps, 1))[:2049] for x in (p, q, want))
        labels = (labels * reps)[:2049]
    same(c.pairing_many(p, q), want, labels, path)


def test_miller_loop_and_line_coefficients(ctx, ctx_tp, pp):
    """miller_loop_many and g2_precompute_many (all 87 line coefficients) of the
    structured pairs.  Both entry points ignore the path thresholds (they run the
    prepare kernel and k_miller), so they run once; the final exponentiation of the
    Miller values then gives the Gt on the 16-lane layout (ctx) and on the step
    machine (ctx_tp)."""
    p, q, labels, want = pp
    f = ctx.miller_loop_many(p, q)
    same(f, np.stack([O.miller_loop_batch(q[k], p[k])[1] for k in range(len(labels))]), labels, "miller_loop_many")
    for name, c in (("16-lane", ctx), ("step machine", ctx_tp)):
        fe, ok = c.final_exponentiation_many(f)
        assert ok.all()
        same(fe, want, labels, "final_exponentiation of the Miller values, " + name)
    coeffs = ctx.g2_precompute_many(q)
    qa, rcs = O.g2_to_affine(q)
    assert rcs == [0] * len(labels)
    same(coeffs, np.stack([O.g2_precompute(qa[k]) for k in range(len(labels))]), labels, "g2_precompute_many")


# ---------------------------------------------------------------- 7. final exponentiation
@pytest.fixture(scope="module")
def fe_inputs(fq12, pp):
    a, labels, _ = fq12
    p, q, pl, _ = pp
    pick = np.linspace(0, len(pl) - 1, 8).astype(int)
    ml = np.stack([O.miller_loop_batch(q[k], p[k])[1] for k in pick])
    f = np.concatenate([a, ml])
    labels = labels + ["Miller value of " + pl[k] for k in pick]
    want, rcs = O.final_exponentiation(f)
    in_fq6 = np.concatenate([E.fq12_subfield_mask(labels[:a.shape[0]]), np.zeros(8, bool)])
    return f, labels, want, np.array(rcs), in_fq6


@pytest.mark.parametrize("path", ["digit_sliced", "wide16", "step_machine"])
def test_final_exponentiation_on_structured_values(fe_inputs, path, monkeypatch):
    """The structured Fq12 rows (subfield rows, 1, -1, single coefficients, zero, ...)
    and eight Miller values through k_fe_ds (batches of at most 256), the 16-lane
    k_fe_wide (BN254MI_FE_DS_MAX=0) and the step machine (fe_wide_max = 0), at
    n = 4, 100 and all rows.  Rows in Fq6 give exactly Fq12::one() with ok = 1 --
    eleven coordinates of the true result are zero --, the zero row ok = 0."""
    f, labels, want, rcs, in_fq6 = fe_inputs
    if path == "wide16":
        monkeypatch.setenv("BN254MI_FE_DS_MAX", "0")
    c = _ctx(fe_wide_max=0 if path == "step_machine" else 1 << 20)
    full = len(labels)
    assert full >= 148 and full <= 256 and in_fq6.sum() >= 20 and labels[0] == "0" and rcs[0] != 0
    assert not rcs[1:].any() and not want[0].any()
    assert np.array_equal(want[in_fq6], np.tile(ONE12, (in_fq6.sum(), 1)))
    cuts = {4: np.array([0, 2, 21, full - 1]), 100: np.r_[0:92, full - 8:full], full: np.arange(full)}
    for n, idx in cuts.items():
        assert len(idx) == n
        lab = [labels[i] for i in idx]
        out, ok = c.final_exponentiation_many(f[idx])
        same(ok[:, None], (rcs[idx] == 0).astype(np.uint8)[:, None], lab, "%s ok n=%d" % (path, n))
        same(out, want[idx], lab, "%s n=%d" % (path, n))
        sub = in_fq6[idx]
        assert sub.any() and np.array_equal(out[sub], np.tile(ONE12, (sub.sum(), 1))) and ok[sub].all()
        assert ok[0] == 0 and not out[0].any()


# ---------------------------------------------------------------- 8. products that are exactly one
@pytest.mark.parametrize("n", [2, 64, 4224])
def test_products_that_are_one(ctx, n):
    """pairing_batch of e(P, Q) e(-P, Q) terms is exactly Gt::one(); 4,224 terms take
    the segmented path with k_seg_tail.  miller_loop_batch against the oracle's
    Miller product."""
    pn, qn = E.one_product_terms(n)
    assert pn.shape[0] == n
    want = O.pairing_batch(pn, qn, nthreads=NT)
    assert np.array_equal(want, ONE12)
    assert np.array_equal(ctx.pairing_batch(pn, qn), want)
    ml = oracle_miller_product(qn, pn)
    if n <= 64:
        assert np.array_equal(ml, O.miller_loop_batch(qn, pn)[1])
    assert np.array_equal(ctx.miller_loop_batch(qn, pn), ml)


def test_products_that_are_one_unfused_tail():
    """The same 4,224 terms with BN254MI_TAIL_FUSED=0 (k_seg_fe1 + k_horner_tree2).
    The library reads the variable once per process, so the call runs in a child
    (tests/edge_probe.py), as tests/failure_probe.py's tail probe does for the
    product library."""
    env = dict(os.environ, BN254MI_TAIL_FUSED="0")
    env.pop("BN254MI_LIB", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "edge_probe.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == {"n": 4224, "code": 0, "is_one": True, "bit_exact": True}, res


# ---------------------------------------------------------------- 9. Gt::pow and the codecs
def test_gt_pow_on_structured_bases_and_scalars(ctx, fq12, pp):
    """{one, -one, the Fq6 rows, four pairing outputs, two Miller values} crossed
    with the whole scalar set (E0(r) in both views, runs of ones, r - 2^k)."""
    a, labels, _ = fq12
    p, q, pl, gt = pp
    sub = E.fq12_subfield_mask(labels)
    pick = [3, 150, 250, len(pl) - 1]
    ml = np.stack([O.miller_loop_batch(q[k], p[k])[1] for k in (5, 300)])
    bases = np.concatenate([a[sub], gt[pick], ml])
    bl = [lab for lab, s in zip(labels, sub) if s] + ["e(%s)" % pl[k] for k in pick] + ["Miller value"] * 2
    assert "1" in bl and "-1" in bl and len(bl) >= 30
    k, kl, _ = E.scalars()
    A = np.repeat(bases, len(kl), axis=0)
    K = np.tile(k, (len(bl), 1))
    lab = ["(%s)^(%s)" % (b, s) for b in bl for s in kl]
    same(ctx.gt_pow_many(A, K), oracle_gt_pow(A, K), lab, "gt_pow")


def test_sqrt_on_e0(ctx):
    """fq_sqrt_many and fq2_sqrt_many on E0(p) in all three views: ok, and the root
    where there is one."""
    a, labels, _ = E.fq_elements()
    out, ok = ctx.fq_sqrt_many(a)
    ref, rok = O.fq_sqrt(a)
    same(ok.astype(bool)[:, None], rok[:, None], labels, "fq_sqrt ok")
    same(out[rok], ref[rok], [lab for lab, s in zip(labels, rok) if s], "fq_sqrt root")
    z = np.zeros_like(a)
    a2 = np.concatenate([np.concatenate([a, z], axis=1), np.concatenate([z, a], axis=1),
                         np.concatenate([a, np.roll(a, -1, axis=0)], axis=1),
                         np.concatenate([a, a], axis=1)])
    l2 = [s % lab for s in ("(%s, 0)", "(0, %s)", "(%s, next)", "(%s, same)") for lab in labels]
    out, ok = ctx.fq2_sqrt_many(a2)
    ref, rok = O.fq2_sqrt(a2)
    same(ok.astype(bool)[:, None], rok[:, None], l2, "fq2_sqrt ok")
    same(out[rok], ref[rok], [lab for lab, s in zip(l2, rok) if s], "fq2_sqrt root")


def test_encodings_next_to_digit_boundaries(ctx):
    """fq_to_big_endian_many on images, fq_from_slice_many and fq2_from_slice_many on
    byte strings, next to every 29-bit digit boundary and 32-bit word boundary
    (2^k - 1, 2^k, 2^k + 1), with E0(p)."""
    items = E.digit_boundary_values() + [("E0 " + lab, v) for lab, v in E.e0(P)]
    labels = [lab for lab, _ in items]
    vals = [v for _, v in items]
    assert len(vals) >= 80
    img = O.ints_to_array(vals).reshape(-1, 4)           # the memory image is v
    same(ctx.fq_to_big_endian_many(img), O.fq_to_big_endian(img), labels, "fq_to_big_endian")
    b = np.stack([be(v) for v in vals] + [be(P), be(P + 1), be((1 << 256) - 1)])
    lb = labels + ["p", "p+1", "2^256-1"]
    out, st = ctx.fq_from_slice_many(b)
    ref, rst = O.fq_from_slice(b)
    assert list(rst[-3:]) == [O.FIELD_NOT_MEMBER] * 3 and not rst[:-3].any()
    same(st[:, None], rst[:, None], lb, "fq_from_slice status")
    same(out, ref, lb, "fq_from_slice")
    same(ctx.fq_to_big_endian_many(ref[:-3]), b[:-3], labels, "to_big_endian(from_slice)")
    nxt = vals[1:] + vals[:1]
    b2 = np.stack([be(c1 * P + c0, 64) for c0, c1 in zip(vals, nxt)] + [be(v, 64) for v in vals] +
                  [be(v * P, 64) for v in vals] + [be(P * P - 1, 64), be(P * P, 64)])
    l2 = ["c0 = %s, c1 = next" % x for x in labels] + ["c0 = %s, c1 = 0" % x for x in labels] + \
         ["c0 = 0, c1 = %s" % x for x in labels] + ["p^2-1", "p^2"]
    out, st = ctx.fq2_from_slice_many(b2)
    ref, rst = O.fq2_from_slice(b2)
    assert rst[-1] == O.FIELD_NOT_MEMBER and not rst[:-1].any()
    same(st[:, None], rst[:, None], l2, "fq2_from_slice status")
    same(out, ref, l2, "fq2_from_slice")


def test_decompression_and_validation_of_structured_points(ctx):
    """g*_from_compressed_many and g*_affine_new_many on the structured affine points,
    both signs of y."""
    g1, l1 = E.g1_affine_jac()
    g2, l2 = E.g2_affine_jac()
    c1, c2 = compress_g1(g1[:, :8]), compress_g2(g2[:, :16])
    assert set(c1[:, 0]) == {2, 3} and set(c2[:, 0]) == {10, 11}
    out, st = ctx.g1_from_compressed_many(c1)
    ref, rst = O.g1_from_compressed(c1, NT)
    assert not rst.any()
    same(st[:, None], rst[:, None], l1, "g1_from_compressed status")
    same(out, ref, l1, "g1_from_compressed")
    same(out, g1, l1, "g1_from_compressed == the point")
    out, st = ctx.g2_from_compressed_many(c2)
    ref, rst = O.g2_from_compressed(c2, NT)
    assert not rst.any()
    same(st[:, None], rst[:, None], l2, "g2_from_compressed status")
    same(out, ref, l2, "g2_from_compressed")
    same(out, g2, l2, "g2_from_compressed == the point")
    out, st = ctx.g1_affine_new_many(g1[:, :4], g1[:, 4:8])
    ref, rst = O.g1_affine_new(g1[:, :4], g1[:, 4:8])
    assert not rst.any()
    same(st[:, None], rst[:, None], l1, "g1_affine_new status")
    same(out, ref, l1, "g1_affine_new")
    _, st = ctx.g1_affine_new_many(g1[:, 4:8], g1[:, :4])  # (y, x)
    _, rst = O.g1_affine_new(g1[:, 4:8], g1[:, :4])
    same(st[:, None], rst[:, None], l1, "g1_affine_new (y, x) status")
    out, st = ctx.g2_affine_new_many(g2[:, :8], g2[:, 8:16])
    ref, rst = O.g2_affine_new(g2[:, :8], g2[:, 8:16], NT)
    assert not rst.any()
    same(st[:, None], rst[:, None], l2, "g2_affine_new status")
    same(out, ref, l2, "g2_affine_new")

