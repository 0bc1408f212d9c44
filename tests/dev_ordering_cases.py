"""Shared by tests/test_dev_ordering_cases.py and tests/test_gpu_dev_ordering.py: the inputs,
the expected values and the "V0 answers" of the cross-stream chains, from the oracle alone.

A chain is two _dev calls: A writes a buffer, B reads it.  Before a chain runs, A's output
buffer holds a VALID value that is not the right one (V0: the G1 or G2 generator, Gt::one()),
so a B that ran before A would still see well-formed data and would return the oracle's answer
for V0 -- `v0` below -- instead of `want`.  The CPU test checks that the two differ, so that
the GPU test can tell them apart."""
import functools

import numpy as np

from oracle import oracle as O
from tests import msm_basis_cases as B
from tests import msm_g2_cases as C2
from tests import msm_many_cases as M
from tests import msm_prepared_cases as C

NT = 16
FRESH = 0xffffffff       # BN_QIDX_FRESH
ZERO_GT = np.zeros(48, np.uint64)


def g1_gen():
    return O.g1_one().copy()


def g2_gen():
    return O.g2_one().copy()


def gt_one():
    a = np.zeros(48, np.uint64)
    a[:4] = O.canon_to_mont_array([1]).reshape(4)
    return a


def products(p, q, off):
    """(m, 48): pairing_batch of the pairs off[j] <= i < off[j + 1]."""
    off = [int(x) for x in off]
    return np.stack([O.pairing_batch(p[a:b], q[a:b]) for a, b in zip(off[:-1], off[1:])])


def full_q(qidx, table, fresh):
    """The G2 point of every term: table[qidx[i]], or the next row of `fresh`."""
    out, f = [], 0
    for i in qidx:
        if int(i) == FRESH:
            out.append(fresh[f])
            f += 1
        else:
            out.append(table[int(i)])
    assert f == len(fresh)
    return np.stack(out)


def _with_row(a, row, value):
    a = a.copy()
    a[row] = value
    return a


@functools.lru_cache(maxsize=None)
def cases():
    """Every chain's data, computed once: a dict of dicts of read-only arrays."""
    pts = M.g1_points(257, 9101)                        # Jacobian images, z != one
    _, ks = O.random_scalars(257, seed=9102, lo=1)
    Q = C2.g2_points(65, 9103)
    _, k2 = O.random_scalars(65, seed=9104, lo=1)
    fixed = M.g1_points(40, 9105)                       # the G1 points beside the computed ones
    c = {}

    # bn_g1_msm_many_dev (5 segments of 2-4 terms, out_stride 2, into the p array) ->
    # bn_pairing_batch_prepared_many_dev (5 two-term products over two prepared points)
    lengths = [2, 4, 3, 2, 4]
    n = sum(lengths)
    off = M.offsets_of(lengths)
    sums = M.expect(pts[:n], ks[:n], off)
    p_v0 = np.zeros((10, 12), np.uint64)
    p_v0[0::2] = g1_gen()
    p_v0[1::2] = fixed[:5]
    p_want = p_v0.copy()
    p_want[0::2] = sums
    qidx = np.tile(np.array([0, 1], np.uint32), 5)
    poff = np.arange(0, 11, 2).astype(np.uintp)
    table = Q[:2]
    c["many_products"] = {
        "p": pts[:n], "k": ks[:n], "off": off, "sums": sums, "pairs_v0": p_v0, "pairs": p_want, "table": table,
        "qidx": qidx, "poff": poff, "want": products(p_want, full_q(qidx, table, []), poff),
        "v0": products(p_v0, full_q(qidx, table, []), poff)}

    # bn_g1_msm_prepared_many_dev (m = 5, k = 3, out_stride 4) -> bn_pairing_batch_prepared_many_dev
    # (5 Groth16-shaped products: vk_x against a prepared point, one fresh pair, two more prepared)
    bases = pts[20:23]
    scal = ks[30:45].reshape(5, 3, 4)
    vkx = C.expect(bases, scal)
    g_v0 = np.zeros((20, 12), np.uint64)
    g_v0[0::4] = g1_gen()
    for r in (1, 2, 3):
        g_v0[r::4] = fixed[5 * r:5 * r + 5]
    g_want = g_v0.copy()
    g_want[0::4] = vkx
    gq = np.tile(np.array([0, FRESH, 1, 2], np.uint32), 5)
    goff = np.arange(0, 21, 4).astype(np.uintp)
    gtable, gfresh = Q[2:5], Q[5:10]
    c["prepared_products"] = {
        "bases": bases, "scal": scal, "sums": vkx, "pairs_v0": g_v0, "pairs": g_want, "table": gtable, "fresh": gfresh,
        "qidx": gq, "poff": goff, "want": products(g_want, full_q(gq, gtable, gfresh), goff),
        "v0": products(g_v0, full_q(gq, gtable, gfresh), goff)}

    # bn_g1_msm_dev / bn_g1_msm_basis_dev (257 terms) -> the sum as p[0] of three pairs
    s1 = B.expect(pts, ks)
    p3_v0 = _with_row(fixed[20:23], 0, g1_gen())
    p3 = _with_row(fixed[20:23], 0, s1)
    q3 = Q[10:13]
    c["msm_pairs"] = {
        "p": pts, "k": ks, "sum": s1, "p3_v0": p3_v0, "p3": p3, "q3": q3,
        "want_batch": O.pairing_batch(p3, q3), "v0_batch": O.pairing_batch(p3_v0, q3),
        "want_miller": O.miller_loop_batch(q3, p3)[1],
        "want_many": O.pairing_many(p3, q3, NT), "v0_many": O.pairing_many(p3_v0, q3, NT)}

    # bn_g2_msm_dev (65 terms) -> the sum as q[0] of three pairs
    s2 = C2.expect(Q, k2)
    q3g_v0 = _with_row(Q[10:13], 0, g2_gen())
    q3g = _with_row(Q[10:13], 0, s2)
    pg = fixed[20:23]
    c["g2msm_pairs"] = {
        "q": Q, "k": k2, "sum": s2, "q3_v0": q3g_v0, "q3": q3g, "p3": pg,
        "want": O.pairing_many(pg, q3g, NT), "v0": O.pairing_many(pg, q3g_v0, NT)}

    # bn_g2_prepare_dev (3 points) -> bn_pairing_prepared_many_dev (7 pairs); the same pairs with
    # one index past the handle's count (that row is the zero image) for the sticky outcome
    qp = Q[13:16]
    p7 = fixed[23:30]
    idx = np.array([0, 1, 2, 2, 1, 0, 1], np.uint32)
    gtp = O.pairing_many(p7, qp[idx], NT)
    bad = idx.copy()
    bad[3] = 3
    c["prepared"] = {"q": qp, "p": p7, "idx": idx, "want": gtp, "bad_idx": bad, "bad_want": _with_row(gtp, 3, ZERO_GT)}

    # bn_g1_bases_prepare_dev (3 bases) -> bn_g1_msm_prepared_many_dev (the rows above);
    # bn_g1_basis_prepare_dev (65 bases) -> bn_g1_msm_basis_dev
    c["basis"] = {"bases": pts[:65], "k": ks[:65], "want": B.expect(pts[:65], ks[:65])}

    # Gt producers -> bn_gt_pow_many_dev
    q7 = Q[16:23]
    gt7 = O.pairing_many(p7, q7, NT)
    kp = ks[50:57]
    one7 = np.tile(gt_one(), (7, 1))
    p11, q11 = fixed[:11], Q[23:34]
    off5 = np.array([0, 2, 5, 6, 9, 11], np.uintp)
    prod5 = products(p11, q11, off5)
    k5 = ks[60:65]
    c["pow"] = {
        "p7": p7, "q7": q7, "gt7": gt7, "k7": kp, "want7": O.gt_pow(gt7, kp), "v0_7": O.gt_pow(one7, kp),
        "p11": p11, "q11": q11, "off5": off5, "prod5": prod5, "k5": k5, "want5": O.gt_pow(prod5, k5),
        "v0_5": O.gt_pow(one7[:5], k5), "want_prepared": O.gt_pow(gtp, kp)}

    # a call that takes no part in the ordering, over buffers of its own
    c["mul"] = {"p": pts[100:133], "k": ks[100:133], "want": O.g1_mul(pts[100:133], ks[100:133], NT)}

    # pinned-upload hand-off: the same entry point twice, with different host control arrays
    p24, q24 = pts[200:224], Q[34:58]
    ox = np.array([0, 3, 5, 9, 12], np.uintp)
    oy = np.array([0, 1, 4, 6, 10, 11, 17], np.uintp)
    qx = np.array([0, 1, 2, FRESH, 2, 1, 0, FRESH, 1, 1, 2, 0], np.uint32)
    qy = np.array([FRESH, 2, 2, 1, 0, FRESH, 1, 0, 2, FRESH, 0, 0, 1, 2, FRESH, 1, 0], np.uint32)
    fx, fy = q24[:2], q24[2:6]
    lx, ly = [2, 4, 3], [3, 1, 4, 2, 5]
    c["handoff"] = {
        "p": p24, "q": q24, "off_x": ox, "off_y": oy, "want_x": products(p24, q24, ox), "want_y": products(p24, q24, oy),
        "table": gtable, "qidx_x": qx, "qidx_y": qy, "fresh_x": fx, "fresh_y": fy,
        "want_px": products(p24, full_q(qx, gtable, fx), ox), "want_py": products(p24, full_q(qy, gtable, fy), oy),
        "mp": pts[:15], "mk": ks[:15], "moff_x": M.offsets_of(lx), "moff_y": M.offsets_of(ly),
        "want_mx": M.expect(pts[:9], ks[:9], M.offsets_of(lx)), "want_my": M.expect(pts[:15], ks[:15], M.offsets_of(ly))}

    # workspace growth while a call is queued: one pair past the pairing workspace's smallest
    # capacity (1024), one term past an MSM workspace sized for five
    c["regrow"] = {"n_pairs": 1025, "msm5": B.expect(pts[:5], ks[:5]), "msm6": B.expect(pts[:6], ks[:6])}

    for d in c.values():
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


# (chain, expected value, V0 answer): what the CPU test compares and the GPU test tells apart
V0_PAIRS = [("many_products", "want", "v0"), ("prepared_products", "want", "v0"), ("msm_pairs", "want_batch", "v0_batch"),
            ("msm_pairs", "want_many", "v0_many"), ("g2msm_pairs", "want", "v0"), ("pow", "want7", "v0_7"),
            ("pow", "want5", "v0_5"), ("pow", "want_prepared", "v0_7")]
