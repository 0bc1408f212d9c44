"""The group law's exceptional branches inside the MI355X kernels, through the C ABI and
bit for bit against the oracle: zero images (z == 0 under any x, y) at every entry point,
G2 * Fr on twist points of order 10069 whose chains pass through zero, res == Q and
res == -Q (tests/group_exceptional_cases.py: chain_events), and the MSMs on families of
bases j * G, j in +-{1..4}, where nearly every reduction step meets an equal or an opposite
point.  The expected MSM rows come from the integer sum of k_i * j_i."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import group_exceptional_cases as X
from tests.codec_util import compress_g2

pytestmark = pytest.mark.gpu
NT = 16
R, ELL = X.R, X.ELL
GROUPS = ("g1", "g2")
WIDTH = X.WIDTH
MUL = {"g1": O.g1_mul, "g2": O.g2_mul}
ORACLE = {
    "g1": {"add": O.g1_add, "sub": O.g1_sub, "neg": O.g1_neg, "normalize": O.g1_normalize, "eq": O.g1_eq},
    "g2": {"add": O.g2_add, "sub": O.g2_sub, "neg": O.g2_neg, "normalize": O.g2_normalize, "eq": O.g2_eq},
}
GT_ONE = np.zeros(48, np.uint64)
GT_ONE[:4] = O.canon_to_mont_array([1]).reshape(4)


@pytest.fixture(scope="module")
def ctx():
    from substrate_bn import Context
    return Context(0)


@pytest.fixture(scope="module")
def ctx_tp():
    """every pairing_many batch on the throughput path (k_pairing_full)"""
    from substrate_bn import Context
    c = Context(0)
    c.set_fe_wide_max(0)
    return c


@pytest.fixture(scope="module")
def ctx_seg():
    """small batches on the segmented latency path with the wide final exponentiation"""
    from substrate_bn import Context
    c = Context(0)
    c.set_latency_max(0)
    return c


@pytest.fixture(scope="module")
def ctx_w2():
    """the one-launch latency path up to 4,096 pairs: the two-wave build above 2,048"""
    from substrate_bn import Context
    c = Context(0)
    c.set_latency_max(4096)
    return c


@pytest.fixture(scope="module")
def pairs():
    p, q, _, _ = O.random_pairs(257, seed=9191, nthreads=NT)
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


def _rows_differ(got, want, labels):
    return [labels[i] for i in range(len(want)) if not np.array_equal(got[i], want[i])][:6]


# ---------------------------------------------------------------- group operators
def _operands(group, pairs):
    """257 rows: every zero image against every zero image, every zero image against nonzero
    points in both positions, then nonzero rows with P + P and P - P among them."""
    zs, zl = X.zero_images(group)
    nz = pairs[0 if group == "g1" else 1]
    a, b, labels = [], [], []
    for i in range(5):
        for j in range(5):
            a.append(zs[i]), b.append(zs[j]), labels.append("%s | %s" % (zl[i], zl[j]))
    for i in range(5):
        for k in range(3):
            a.append(zs[i]), b.append(nz[5 * k + i]), labels.append("%s | P%d" % (zl[i], 5 * k + i))
            a.append(nz[5 * k + i]), b.append(zs[i]), labels.append("P%d | %s" % (5 * k + i, zl[i]))
    k = 0
    while len(a) < 257:
        a.append(nz[k])
        b.append(nz[k] if k % 7 == 0 else ORACLE[group]["neg"](nz[k:k + 1])[0] if k % 7 == 1 else nz[256 - k])
        labels.append("P%d | row %d" % (k, k))
        k += 1
    return np.stack(a), np.stack(b), labels


def _want(group, op, a, b):
    if op == "eq":
        return np.array(ORACLE[group]["eq"](a, b), np.uint8)
    return ORACLE[group][op](a) if op in ("neg", "normalize") else ORACLE[group][op](a, b)


@pytest.mark.parametrize("group", GROUPS)
def test_group_ops_on_zero_images(ctx, pairs, group):
    """bn_{g1,g2}_{add,sub,neg,normalize,eq}_many, host form and _dev in place."""
    import torch
    dev = torch.device("cuda", 0)
    a, b, labels = _operands(group, pairs)
    n, w = a.shape
    assert n == 257
    s = torch.cuda.Stream(dev)
    for op in ("add", "sub", "neg", "normalize", "eq"):
        want = _want(group, op, a, b)
        got = ctx.group_op_many(group, op, a, b)
        assert not _rows_differ(got, want, labels), (op, _rows_differ(got, want, labels))
        da = torch.from_numpy(a.view(np.int64)).to(dev)
        db = torch.from_numpy(b.view(np.int64)).to(dev)
        out = torch.full((n,), 7, dtype=torch.uint8, device=dev) if op == "eq" else da   # in place: out aliases a
        torch.cuda.synchronize(dev)
        ctx.group_op_many_dev(group, op, da.data_ptr(), db.data_ptr(), n, out.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize(dev)
        got = out.cpu().numpy() if op == "eq" else out.cpu().numpy().view(np.uint64)
        assert not _rows_differ(got, want, labels), ("dev", op, _rows_differ(got, want, labels))
    # the second operand in place as well
    db = torch.from_numpy(b.view(np.int64)).to(dev)
    da = torch.from_numpy(a.view(np.int64)).to(dev)
    torch.cuda.synchronize(dev)
    ctx.group_op_many_dev(group, "add", da.data_ptr(), db.data_ptr(), n, db.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(db.cpu().numpy().view(np.uint64), _want(group, "add", a, b))


# ---------------------------------------------------------------- scalar multiplication of zero images
def _zero_mul_rows(group, pairs):
    zs, zl = X.zero_images(group)
    nz = pairs[0 if group == "g1" else 1]
    p, ks, labels = [], [], []
    for lab, k in X.zero_image_scalars():
        for i in range(5):
            p.append(zs[i]), ks.append(k), labels.append("%s * %s" % (zl[i], lab))
    g = O.SplitMix64(X.SEED + 200)
    i = 0
    while len(p) < 257:
        p.append(nz[i]), ks.append(g.below(R)), labels.append("P%d * random" % i)
        i += 1
    order = np.random.default_rng(3).permutation(len(p))         # zero images and chains mixed in every wave
    return np.stack(p)[order][:257], [ks[i] for i in order][:257], [labels[i] for i in order][:257]


@pytest.mark.parametrize("group", GROUPS)
def test_mul_many_on_zero_images(ctx, pairs, group):
    p, ks, labels = _zero_mul_rows(group, pairs)
    assert p.shape[0] == 257 and sum(bool(X.is_zero(r)) for r in p) >= 150
    K = X.fr(ks)
    want = MUL[group](p, K, NT)
    got = ctx.g1_mul_many(p, K) if group == "g1" else ctx.g2_mul_many(p, K)
    assert not _rows_differ(got, want, labels), _rows_differ(got, want, labels)
    # the rule itself on the kernel's output: z stays 0 for every zero image
    assert all(bool(X.is_zero(got[i])) for i in range(257) if X.is_zero(p[i]))


def _plant_zero_rows(base, S, rows):
    zs, _ = X.zero_images("g1")
    sc = [k for _, k in X.zero_image_scalars()]
    for t, row in enumerate(rows):
        base[row] = zs[t % 5]
        S[row] = X.fr([sc[(7 * t) % len(sc)]])[0]


def test_g1_mul_two_chain_kernel_with_zero_images(ctx):
    """k_g1_mul2 (lane i runs rows i and i + h) at 2^18 + 3 rows: zero images in the first
    half, in the second half and in the last row, random rows elsewhere."""
    n = (1 << 18) + 3
    h = (n + 1) // 2
    _, S = O.random_scalars(n, seed=9444, lo=0)
    base = ctx.g1_mul_many(np.tile(O.g1_one(), (n, 1)), np.roll(S, 11, axis=0))
    planted = [i for i in range(1, 40, 2)] + [h + i for i in range(0, 40, 3)] + [h - 1, n - 1, 64, h + 64, 65, h + 65]
    _plant_zero_rows(base, S, planted)
    got = ctx.g1_mul_many(base, S)
    rows = np.unique(np.r_[0:48, 60:70, h - 24:h + 70, n - 24:n])
    assert len(rows) <= 200 and set(planted) <= set(rows.tolist())
    want = O.g1_mul(base[rows], S[rows], NT)
    bad = [int(r) for r, g, w in zip(rows, got[rows], want) if not np.array_equal(g, w)]
    assert not bad, bad[:8]


def test_g1_mul_512_thread_launch_with_zero_images(ctx):
    """k_g1_mul in 512-thread blocks (131,072 rows: every CU gets one such block)."""
    n = 131072
    _, S = O.random_scalars(n, seed=9445, lo=0)
    base = ctx.g1_mul_many(np.tile(O.g1_one(), (n, 1)), np.roll(S, 5, axis=0))
    planted = list(range(0, 64, 3)) + list(range(500, 530, 2)) + [n - 1, n - 64, n // 2, n // 2 + 1]
    _plant_zero_rows(base, S, planted)
    got = ctx.g1_mul_many(base, S)
    rows = np.unique(np.r_[0:64, 496:532, n // 2 - 8:n // 2 + 8, n - 70:n])
    assert len(rows) <= 200 and set(planted) <= set(rows.tolist())
    want = O.g1_mul(base[rows], S[rows], NT)
    bad = [int(r) for r, g, w in zip(rows, got[rows], want) if not np.array_equal(g, w)]
    assert not bad, bad[:8]


# ---------------------------------------------------------------- G2 * Fr on points of order ELL
def test_g2_mul_many_on_order_ell_points(ctx):
    """The constructed and the uniform scalar families on Q in both scalings, then the
    constructed ones with the scalings swapped, then j * Q under uniform scalars: 512 rows,
    the raw Jacobian image against the oracle."""
    pts, plabels, _ = X.order_ell_points()
    fam = X.order_ell_scalars()
    p, ks, labels = [], [], []
    i = 0
    for name, rows in fam.items():
        for lab, k in rows:
            p.append(pts[i % 2]), ks.append(k), labels.append("%s | %s" % (plabels[i % 2], lab))
            i += 1
    for name in ("same", "cancel", "multiple"):
        for lab, k in fam[name]:
            assert X.chain_events(k), lab
            p.append(pts[(i + 1) % 2]), ks.append(k), labels.append("%s | %s" % (plabels[(i + 1) % 2], lab))
            i += 1
    g = O.SplitMix64(X.SEED + 300)
    while len(p) < 512:
        j = len(p) % len(pts)
        p.append(pts[j]), ks.append(g.below(R)), labels.append("%s | uniform" % plabels[j])
    p, K = np.stack(p), X.fr(ks)
    assert p.shape[0] == 512
    want = O.g2_mul(p, K, NT)
    got = ctx.g2_mul_many(p, K)
    assert not _rows_differ(got, want, labels), _rows_differ(got, want, labels)
    for img, k in zip(got, ks):
        assert bool(X.is_zero(img)) == (k % ELL == 0)


# ---------------------------------------------------------------- pairing entry points
def _planted_pairs(pairs, n):
    """n pairs with every zero image in the P slot, in the Q slot and in both, first rows
    and last rows; (p, q, labels)."""
    p, q = pairs[0][:n].copy(), pairs[1][:n].copy()
    z1, zl = X.zero_images("g1")
    z2, _ = X.zero_images("g2")
    labels = ["pair %d" % i for i in range(n)]
    slots = [(i, "P") for i in range(5)] + [(i, "Q") for i in range(5)] + [(i, "PQ") for i in range(5)]
    rows = ([1, 3, 4, 6] if n < 16 else list(range(1, 30, 2))) + [n - 1]
    for t, row in enumerate(rows):
        i, where = slots[(t * 4) % len(slots)] if n < 16 else slots[t % len(slots)]
        if row == n - 1:
            i, where = 4, "PQ"
        if "P" in where:
            p[row] = z1[i]
        if "Q" in where:
            q[row] = z2[(i + (2 if where == "PQ" else 0)) % 5]
        labels[row] = "%s: %s" % (where, zl[i])
    return p, q, labels


@pytest.fixture(scope="module")
def pairing_cases(pairs):
    out = {}
    for n in (9, 65, 257):
        p, q, labels = _planted_pairs(pairs, n)
        out[n] = (p, q, labels, O.pairing_many(p, q, NT))
    return out


@pytest.mark.parametrize("n", [9, 65, 257])
def test_pairing_many_with_zero_images(ctx, ctx_seg, ctx_tp, ctx_w2, pairing_cases, n):
    p, q, labels, want = pairing_cases[n]
    nzero = sum(np.array_equal(r, GT_ONE) for r in want)
    assert (5 if n == 9 else 16) <= nzero < n
    for name, c in (("latency", ctx), ("segmented, wide final exponentiation", ctx_seg), ("throughput", ctx_tp),
                    ("latency to 4096", ctx_w2)):
        got = c.pairing_many(p, q)
        assert not _rows_differ(got, want, labels), (name, _rows_differ(got, want, labels))


def test_pairing_many_two_wave_kernel_with_zero_images(ctx_w2, pairs, pairing_cases):
    """2,049 pairs: k_pairing_latency_w2.  The 257 planted pairs tiled, so the expected rows
    are those of the 257."""
    p, q, labels, want = pairing_cases[257]
    n = 2049
    reps = n // 257 + 1
    pp, qq = np.tile(p, (reps, 1))[:n], np.tile(q, (reps, 1))[:n]
    ww = np.tile(want, (reps, 1))[:n]
    got = ctx_w2.pairing_many(pp, qq)
    bad = [i for i in range(n) if not np.array_equal(got[i], ww[i])]
    assert not bad, [(i, labels[i % 257]) for i in bad[:6]]


def test_miller_loop_many_with_zero_images(ctx, ctx_tp, pairing_cases):
    p, q, labels, _ = pairing_cases[65]
    want = np.stack([GT_ONE if (X.is_zero(p[k]) or X.is_zero(q[k])) else O.miller_loop_batch(q[k], p[k])[1]
                     for k in range(65)])
    for name, c in (("default", ctx), ("throughput", ctx_tp)):
        got = c.miller_loop_many(p, q)
        assert not _rows_differ(got, want, labels), (name, _rows_differ(got, want, labels))


def _products_of_four(pairs):
    """Products of 4 terms with one zero-image term each, and the products of the other 3:
    (p, q, offsets, p3, q3, offsets3, labels)."""
    z1, zl = X.zero_images("g1")
    z2, _ = X.zero_images("g2")
    P, Q = pairs
    p, q, p3, q3, labels = [], [], [], [], []
    t = 0
    for where in ("P", "Q", "PQ"):
        for i in range(5):
            rows = [4 * t + k for k in range(4)]
            slot = (t + i) % 4
            for k, r in enumerate(rows):
                zp = k == slot and "P" in where
                zq = k == slot and "Q" in where
                p.append(z1[i] if zp else P[r])
                q.append(z2[(i + 1) % 5] if zq else Q[r])
                if k != slot:
                    p3.append(P[r]), q3.append(Q[r])
            labels.append("%s in term %d: %s" % (where, slot, zl[i]))
            t += 1
    m = len(labels)
    off = np.arange(0, 4 * m + 1, 4).astype(np.uintp)
    off3 = np.arange(0, 3 * m + 1, 3).astype(np.uintp)
    return np.stack(p), np.stack(q), off, np.stack(p3), np.stack(q3), off3, labels


@pytest.fixture(scope="module")
def products(pairs):
    p, q, off, p3, q3, off3, labels = _products_of_four(pairs)
    want = np.stack([O.pairing_batch(p3[3 * j:3 * j + 3], q3[3 * j:3 * j + 3]) for j in range(len(labels))])
    want4 = np.stack([O.pairing_batch(p[4 * j:4 * j + 4], q[4 * j:4 * j + 4]) for j in range(len(labels))])
    assert np.array_equal(want, want4)          # the oracle skips the zero-image term
    return p, q, off, labels, want


def test_pairing_batch_and_batch_many_skip_zero_image_terms(ctx, products):
    from substrate_bn import Context
    p, q, off, labels, want = products
    for j, lab in enumerate(labels):
        assert np.array_equal(ctx.pairing_batch(p[4 * j:4 * j + 4], q[4 * j:4 * j + 4]), want[j]), lab
    own = Context(0)
    for pmin in (0, 1 << 20):                   # the packed kernel, and one product at a time
        own.set_products_min(pmin)
        got = own.pairing_batch_many(p, q, off)
        assert not _rows_differ(got, want, labels), (pmin, _rows_differ(got, want, labels))
    own.close()
    # one product of all 60 terms: 15 of them skipped
    assert np.array_equal(ctx.pairing_batch(p, q), O.pairing_batch(p, q))


def test_prepared_g2_with_zero_images(ctx, pairs, products):
    """bn_g2_prepare on zero images: pairs against such a q[j] give Gt::one() (its zero flag),
    in bn_pairing_prepared_many, bn_miller_loop_prepared_many and as a term of
    bn_pairing_batch_prepared_many."""
    from substrate_bn import _native
    z2, zl = X.zero_images("g2")
    P, Q = pairs
    prepared = np.concatenate([Q[:3], z2, Q[3:4]])              # 3 points, 5 zero images, 1 point
    qi = [0, 1, 2, None, None, None, None, None, 3]
    h = ctx.g2_prepare(prepared)
    try:
        assert ctx.g2_prepared_count(h) == 9
        p = np.concatenate([P[:63], X.zero_images("g1")[0][:2]])   # 65 pairs, two zero images in the P slot
        idx = np.array([(5 * i) % 9 for i in range(65)], np.uint32)
        want = O.pairing_many(p, prepared[idx], NT)
        for i in range(65):
            if qi[idx[i]] is None:
                assert np.array_equal(want[i], GT_ONE)
        got = ctx.pairing_prepared_many(p, h, idx)
        bad = [i for i in range(65) if not np.array_equal(got[i], want[i])]
        assert not bad, [(i, int(idx[i])) for i in bad[:6]]
        ml = ctx.miller_loop_prepared_many(p, h, idx)
        assert np.array_equal(ml, ctx.miller_loop_many(p, prepared[idx]))
        assert all(np.array_equal(ml[i], GT_ONE) for i in range(65) if qi[idx[i]] is None or i >= 63)
        # products of 4: the zero-image term prepared, fresh, or a zero image in the P slot of a prepared term
        pp, qq, off, labels, want = products
        m = len(labels)
        qidx = np.full(4 * m, _native.QIDX_FRESH, np.uint32)
        want_rows = []
        p_terms = pp.copy()
        fresh = []
        for j in range(m):
            for k in range(4):
                t = 4 * j + k
                if X.is_zero(qq[t]) and j % 2 == 0:
                    qidx[t] = 3 + (j % 5)                        # a prepared zero image
                elif not X.is_zero(qq[t]) and k == 3:
                    qidx[t] = [0, 1, 2, 8][j % 4]                # a prepared point
                else:
                    fresh.append(qq[t])
            full = [prepared[qidx[4 * j + k]] if qidx[4 * j + k] != _native.QIDX_FRESH else qq[4 * j + k] for k in range(4)]
            want_rows.append(O.pairing_batch(p_terms[4 * j:4 * j + 4], np.stack(full)))
        got = ctx.pairing_batch_prepared_many(p_terms, np.stack(fresh), h, qidx, off)
        assert not _rows_differ(got, np.stack(want_rows), labels), _rows_differ(got, np.stack(want_rows), labels)
    finally:
        ctx.g2_prepared_destroy(h)


def test_entry_points_that_fail_on_zero_images(ctx, pairs):
    """bn_miller_loop_batch and bn_g2_precompute_many return BN_ERR_TO_AFFINE where the
    reference's to_affine fails, for every zero image in either slot."""
    from substrate_bn import BnError, _native
    P, Q = pairs
    z1, zl = X.zero_images("g1")
    z2, _ = X.zero_images("g2")
    for i in range(5):
        for where in ("P", "Q"):
            p, q = P[:3].copy(), Q[:3].copy()
            if where == "P":
                p[i % 3] = z1[i]
            else:
                q[i % 3] = z2[i]
            assert O.miller_loop_batch(q, p)[0] == 1
            with pytest.raises(BnError) as e:
                ctx.miller_loop_batch(q, p)
            assert e.value.code == _native.BN_ERR_TO_AFFINE, (where, zl[i])
        q = Q[:4].copy()
        q[(i + 1) % 4] = z2[i]
        with pytest.raises(BnError) as e:
            ctx.g2_precompute_many(q)
        assert e.value.code == _native.BN_ERR_TO_AFFINE, zl[i]
    rc, want = O.miller_loop_batch(Q[:3], P[:3])                  # the context stays usable
    assert rc == 0 and np.array_equal(ctx.miller_loop_batch(Q[:3], P[:3]), want)


# ---------------------------------------------------------------- MSMs
def _msm_ways(group):
    from tests import test_gpu_msm, test_gpu_msm_g2
    return (test_gpu_msm if group == "g1" else test_gpu_msm_g2)._all_ways


@pytest.mark.parametrize("family", range(6))
@pytest.mark.parametrize("group", GROUPS)
def test_msm_on_dense_families(ctx, group, family):
    """bn_g1_msm / bn_g2_msm: the bucket path at c = 2, 5 and automatic, the _dev form and
    the small path."""
    name, p, ks, want = X.dense_families(group)[family]
    got = _msm_ways(group)(ctx, p, X.fr(ks))
    assert len(got) == 5
    bad = [way for way, out in got.items() if not np.array_equal(out, want)]
    assert not bad, (name, bad)


def test_g2_msm_in_the_group_of_order_ell(ctx):
    p, ks, want, s = X.order_ell_msm()
    assert X.model_point(want) == X.model_mul(s, X.model_point(X.order_ell_q()))
    got = _msm_ways("g2")(ctx, p, X.fr(ks))
    bad = [way for way, out in got.items() if not np.array_equal(out, want)]
    assert {"small", "bucket c=2", "bucket c=5", "bucket c=0", "dev"} == set(got) and not bad, bad


@pytest.mark.parametrize("unit", [2, 16])
def test_g1_msm_many_on_dense_segments(ctx, unit):
    """bn_g1_msm_many: every width with every unit setting, launch sets of 64 terms, _dev."""
    from tests import test_gpu_msm_many as T
    p, ks, off, want = X.many_segments(unit)
    try:
        got = T._all_ways(ctx, p, X.fr(ks), off)
        ctx.set_msm_many_unit(unit)
        got["unit %d, default width" % unit] = ctx.g1_msm_many(p, X.fr(ks), off)
    finally:
        T._defaults(ctx)
    for way, out in got.items():
        bad = [j for j in range(len(want)) if not np.array_equal(out[j], want[j])]
        assert not bad, (way, bad[:8])


@pytest.mark.parametrize("c", [4, 0])
def test_g1_msm_prepared_many_on_colliding_bases(ctx, c):
    """bn_g1_msm_prepared_many over [G, G rescaled, -G, 2G, -2G, G, a zero image] at widths 4
    and the default, with 1, 2, 64 and automatic lanes and the _dev form."""
    from tests import test_gpu_msm_prepared as T
    bases, rows, want = X.prepared_case(c or T.DEFAULT_C)
    scal = X.fr([v for row in rows for v in row]).reshape(len(rows), 7, 4)
    h = ctx.g1_bases_prepare(bases, c)
    try:
        assert ctx.g1_prepared_window(h) == (c or T.DEFAULT_C)
        for way, out in T._all_ways(ctx, h, scal).items():
            bad = [j for j in range(len(rows)) if not np.array_equal(out[j], want[j])]
            assert not bad, (way, bad[:8], rows[bad[0]])
    finally:
        ctx.g1_prepared_destroy(h)


# ---------------------------------------------------------------- small-order input to the decoders and the pairing
@pytest.fixture(scope="module")
def outside_subgroup():
    """Twist points outside the subgroup: j * Q of order ELL, and Q + S, S in the subgroup.
    ((n, 24) normalized images, labels)."""
    pts, plabels, js = X.order_ell_points()
    s = O.g2_mul(O.g2_one(), X.fr([3, 0x1234567, R - 2]))
    mixed = O.g2_add(np.stack([pts[0], pts[5], pts[8]]), s)
    rows = O.g2_normalize(np.concatenate([pts[0::2], mixed]))
    labels = plabels[0::2] + ["Q + S #%d" % i for i in range(3)]
    for j in js:
        assert j % ELL and R % ELL          # order ELL (a prime) does not divide r: none lies in the subgroup
    return rows, labels


def test_decoders_reject_small_order_points(ctx, outside_subgroup):
    """bn_g2_affine_new_many: NOT_IN_SUBGROUP.  bn_g2_from_compressed_many: the same failure of
    AffineG2::new, which G2::from_compressed reports as CurveError::NotMember (lib.rs:525);
    the points are on the curve, so the order check alone rejects them."""
    rows, labels = outside_subgroup
    x, y = np.ascontiguousarray(rows[:, :8]), np.ascontiguousarray(rows[:, 8:16])
    _, st_o = O.g2_affine_new(x, y)
    _, st = ctx.g2_affine_new_many(x, y)
    assert list(st_o) == [O.GROUP_NOT_IN_SUBGROUP] * len(labels)
    assert list(st) == list(st_o), [lab for lab, s in zip(labels, st) if s != O.GROUP_NOT_IN_SUBGROUP]
    rec = compress_g2(np.ascontiguousarray(rows[:, :16]))
    _, st_o = O.g2_from_compressed(rec)
    _, st = ctx.g2_from_compressed_many(rec)
    assert list(st_o) == [O.CURVE_NOT_MEMBER] * len(labels)
    assert list(st) == list(st_o), [lab for lab, s in zip(labels, st) if s != O.CURVE_NOT_MEMBER]
    assert all(X.model_on_curve(X.model_point(r)) for r in rows)


def test_pairing_many_with_q_outside_the_subgroup(ctx, ctx_tp, pairs, outside_subgroup):
    rows, labels = outside_subgroup
    pts, plabels, _ = X.order_ell_points()
    q = np.concatenate([rows, pts[1::2]])                         # normalized and Jacobian images
    labels = labels + plabels[1::2]
    p = pairs[0][:len(q)]
    want = O.pairing_many(p, q, NT)
    for name, c in (("default", ctx), ("throughput", ctx_tp)):
        got = c.pairing_many(p, q)
        assert not _rows_differ(got, want, labels), (name, _rows_differ(got, want, labels))
