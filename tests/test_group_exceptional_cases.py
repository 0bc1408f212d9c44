"""The generators of tests/group_exceptional_cases.py pinned, the oracle's treatment of zero
images (z == 0 under any x, y) pinned against the rules of groups/mod.rs:246-350, and the
device headers' group law on those inputs through their host compilations (tests/native):
jac_mul on zero images and on twist points of order 10069, the bucket pipeline, the
prepared-bases pipeline and the fresh-bases pipeline on the dense-collision families.
CPU only."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import group_exceptional_cases as X
from tests.native import hostemul as H
from tests.native import msmfixedemul, msmg2emul, msmmanyemul

R, ELL = X.R, X.ELL
GROUPS = ("g1", "g2")
ADD = {"g1": O.g1_add, "g2": O.g2_add}
NEG = {"g1": O.g1_neg, "g2": O.g2_neg}
MUL = {"g1": O.g1_mul, "g2": O.g2_mul}
NORM = {"g1": O.g1_normalize, "g2": O.g2_normalize}
EQ = {"g1": O.g1_eq, "g2": O.g2_eq}
DOUBLE = {"g1": "orc_g1_double", "g2": "orc_g2_double"}


def _double(group, a, times=1):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, X.WIDTH[group])
    for _ in range(times):
        a = O.unary(DOUBLE[group], a, X.WIDTH[group])[0]
    return a


def _nonzero(group, n=4):
    return MUL[group](O.g1_one() if group == "g1" else O.g2_one(), X.fr([5 + 3 * i for i in range(n)]))


# ---------------------------------------------------------------- the generators
def test_order_ell_points():
    q = X.order_ell_q()
    assert not X.is_zero(q) and X.is_zero(O.g2_mul(q, X.fr([ELL]))[0])
    assert R % ELL != 0 and X.H2 % ELL == 0 and (X.H2 // ELL) % ELL != 0
    qa = X.model_point(q)
    assert X.model_on_curve(qa) and X.model_mul(ELL, qa) is None and X.model_mul(ELL - 1, qa) is not None
    pts, labels, js = X.order_ell_points()
    for img, lab, j in zip(pts, labels, js):
        assert not X.is_zero(img), lab
        assert X.model_point(img) == X.model_mul(j, qa), lab
    assert O.g2_eq(pts[0::2], pts[1::2]) == [True] * (len(js) // 2)      # the same points,
    assert not any(np.array_equal(a, b) for a, b in zip(pts[0::2], pts[1::2]))  # other images


def test_chain_events_per_family():
    """Every constructed family reaches its events on every row: none can go vacuous."""
    fam = X.order_ell_scalars()
    for lab, k in fam["same"]:
        assert "same" in X.event_kinds(k), lab
    for lab, k in fam["cancel"]:
        ev = X.chain_events(k)
        kinds = [kind for _, kind in ev]
        assert {"cancel", "double_of_zero", "zero_plus"} <= set(kinds), lab
        assert kinds.index("cancel") < kinds.index("double_of_zero") < kinds.index("zero_plus"), lab
    for lab, k in fam["multiple"]:
        assert k % ELL == 0 and X.event_kinds(k) & {"cancel", "double_of_zero"}, lab
    assert len(fam["uniform"]) == 256
    counts = X.event_counts()
    assert counts["same"]["same"] == len(fam["same"]) and counts["cancel"]["cancel"] == len(fam["cancel"])
    assert X.chain_events(ELL + 2) == [(0, "same")]
    assert X.chain_events((ELL << 2) + 1) == [(2, "cancel"), (1, "double_of_zero"), (0, "double_of_zero"), (0, "zero_plus")]
    assert X.chain_events(5, ell=ELL) == []


@pytest.fixture(scope="module")
def ell_rows():
    """Every constructed scalar and the uniform ones against Q in both scalings, with the
    oracle's products: (points, labels, canonical scalars, oracle images)."""
    pts, plabels, _ = X.order_ell_points()
    labels, ks, rows = [], [], []
    i = 0
    for name, fam in X.order_ell_scalars().items():
        for lab, k in fam:
            labels.append("%s | %s" % (plabels[i % 2], lab))
            rows.append(pts[i % 2])
            ks.append(k)
            i += 1
    p = np.stack(rows)
    return p, labels, ks, O.g2_mul(p, X.fr(ks), nthreads=8)


def test_oracle_g2_mul_on_order_ell_points(ell_rows):
    """z == 0 exactly when ELL | k, and the normalized result is the affine model's."""
    p, labels, ks, prod = ell_rows
    qa = X.model_point(X.order_ell_q())
    small = {}
    for lab, k, img in zip(labels, ks, prod):
        assert bool(X.is_zero(img)) == (k % ELL == 0), lab
        m = k % ELL
        if m not in small:
            small[m] = X.model_mul(m, qa)
        assert X.model_point(img) == small[m], lab


def test_dense_family_expectations_match_a_tree_of_oracle_additions():
    """The integer expectation against the oracle's own sum on a cut of the random family."""
    from tests import msm_g2_cases as C2
    from tests import msm_many_cases as C1
    js, ks = X.random_small_multiples(48, 9, zeros=5)
    for group, exp in (("g1", lambda p, k: C1.expect(p, k, C1.offsets_of([len(p)]))[0]), ("g2", C2.expect)):
        p = X.small_multiple_points(group, js, 9)
        assert np.array_equal(X.expected_sum(group, js, ks), exp(p, X.fr(ks))), group
    js, ks = X.random_small_multiples(48, 9, True)
    assert np.array_equal(X.expected_sum("g1", js, ks), X.zero("g1"))


# ---------------------------------------------------------------- the oracle on zero images
@pytest.mark.parametrize("group", GROUPS)
def test_oracle_zero_image_rules(group):
    zs, labels = X.zero_images(group)
    a = _nonzero(group, len(zs))
    assert X.is_zero(zs).all() and not X.is_zero(a).any()
    assert np.array_equal(ADD[group](a, zs), a)                   # a + (x, y, 0) is a's image
    assert np.array_equal(ADD[group](zs, a), a)
    for i, lab in enumerate(labels):                              # zero + zero: the second operand's image
        second = np.roll(zs, i, axis=0)
        assert np.array_equal(ADD[group](zs, second), second), lab
    assert np.array_equal(NEG[group](zs), zs)                     # neg leaves a zero image untouched
    assert np.array_equal(NORM[group](zs), zs)                    # normalize keeps it
    for i in range(len(zs)):                                      # eq looks only at z
        assert EQ[group](zs, np.roll(zs, i, axis=0)) == [True] * len(zs)
    assert EQ[group](zs, a) == [False] * len(zs) and EQ[group](a, zs) == [False] * len(zs)


@pytest.mark.parametrize("group", GROUPS)
def test_oracle_scalar_times_zero_image_is_repeated_doubling(group):
    """k * (x, y, 0) == double^t((x, y, 0)), t the trailing zero bits of k; k == 0 gives
    (0, one, 0).  double() has no zero check (mod.rs:250-269): checked against add(a, a) on
    nonzero points, where the doubling branch calls it."""
    a = _nonzero(group)
    assert np.array_equal(_double(group, a), ADD[group](a, a))
    zs, labels = X.zero_images(group)
    for lab, k in X.zero_image_scalars():
        got = MUL[group](zs, X.fr([k] * len(zs)))
        want = _double(group, zs, X.trailing_zeros(k)) if k else np.tile(X.zero(group), (len(zs), 1))
        assert np.array_equal(got, want), lab
        assert X.is_zero(got).all()
    moved = _double(group, zs[1:2])[0]
    assert not np.array_equal(moved, zs[1])                       # a zero image keeps evolving its x, y


def test_oracle_pairing_entry_points_on_zero_images():
    p, q, _, _ = O.random_pairs(5, seed=99)
    z1, _ = X.zero_images("g1")
    z2, _ = X.zero_images("g2")
    one = np.zeros(48, np.uint64)
    one[:4] = O.canon_to_mont_array([1]).reshape(4)
    for pp, qq in ((z1, q), (p, z2), (z1, z2)):
        assert np.array_equal(O.pairing_many(pp, qq), np.tile(one, (5, 1)))
        assert np.array_equal(O.pairing_batch(pp, qq), one)
        assert O.miller_loop_batch(qq, pp)[0] == 1                # ToAffineConversion
    for i in range(5):
        pp, qq = p[:4].copy(), q[:4].copy()
        pp[1] = z1[i]
        keep = [0, 2, 3]
        assert np.array_equal(O.pairing_batch(pp, qq), O.pairing_batch(p[keep], q[keep]))


# ---------------------------------------------------------------- jac_mul compiled for the host
def _he_mul(group, p, k):
    return H.call("he_%s_mul" % group, p, O.ints_to_array([k]), out_words=2 * X.WIDTH[group])


@pytest.mark.parametrize("group", GROUPS)
def test_host_jac_mul_on_zero_images(group):
    zs, labels = X.zero_images(group)
    rows = X.zero_image_scalars()
    for i, (lab, k) in enumerate(rows):
        for zi in {i % len(zs), (i + 2) % len(zs)}:
            want = MUL[group](zs[zi], X.fr([k]))[0]
            assert np.array_equal(_he_mul(group, zs[zi], k), want), (labels[zi], lab)


def test_host_jac_mul_on_order_ell_points(ell_rows):
    """Every constructed row, and the uniform rows that meet an event plus the first eight."""
    p, labels, ks, prod = ell_rows
    ran = {kind: 0 for kind in X.KINDS}
    n_uniform = 0
    for img, lab, k, want in zip(p, labels, ks, prod):
        kinds = X.event_kinds(k)
        if "uniform" in lab:
            n_uniform += 1
            if not kinds and n_uniform > 8:
                continue
        assert np.array_equal(_he_mul("g2", img, k), want), lab
        for kind in kinds:
            ran[kind] += 1
    assert all(ran.values()), ran


# ---------------------------------------------------------------- the MSM pipelines compiled for the host
@pytest.mark.parametrize("group", GROUPS)
def test_host_bucket_pipeline_on_dense_families(group):
    for name, p, ks, want in X.dense_families(group):
        for c in (2, 5):
            if group == "g2" and c == 2 and p.shape[0] > 900:
                continue                                          # (the G1 instance runs it)
            assert np.array_equal(msmg2emul.msm(group, p, ks, c), want), (name, c)


def test_host_bucket_pipeline_on_the_order_ell_msm():
    p, ks, want, s = X.order_ell_msm()
    qa = X.model_point(X.order_ell_q())
    assert X.model_point(want) == X.model_mul(s, qa) and not X.is_zero(want)
    for c in (2, 5, 9):
        assert np.array_equal(msmg2emul.msm("g2", p, ks, c), want), c


@pytest.mark.parametrize("c", [4, 10])
def test_host_prepared_pipeline_on_colliding_bases(c):
    bases, rows, want = X.prepared_case(c)
    for lanes in (1, 2, msmfixedemul.lib().msm_fixed_emul_auto_lanes(len(rows), 7, c)):
        got = msmfixedemul.msm_many(bases, rows, c, lanes)
        bad = [j for j in range(len(rows)) if not np.array_equal(got[j], want[j])]
        assert not bad, (lanes, bad, [rows[j] for j in bad[:2]])


@pytest.mark.parametrize("unit", [2, 16])
def test_host_many_pipeline_on_dense_segments(unit):
    p, ks, off, want = X.many_segments(unit)
    for c, u in ((4, unit), (4, 0), (2, unit), (8, 1)):
        got = msmmanyemul.msm_many(p, ks, off, c, u)
        bad = [j for j in range(len(want)) if not np.array_equal(got[j], want[j])]
        assert not bad, (c, u, bad[:8])
