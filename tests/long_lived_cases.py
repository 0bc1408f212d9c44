"""Shared by tests/test_long_lived_cases.py and tests/test_gpu_long_lived.py: the script that one
long-lived context runs -- every kind of call, at sizes that go up and down, with settings
changed and put back, handles made and destroyed and failures in between -- and the oracle's
answer for every step.  CPU only, oracle only, every input and the order from one SplitMix64
seed (SEED).

The script is a list of UNITS, each a short list of steps whose inner order is fixed: a setting,
the calls that run under it and the step that puts it back; a handle, its users and its
destroy call; an outcome step and the call of another kind that must not see its outcome; the
calls that share a buffer and therefore have to meet.  The order of the units is a seeded
shuffle, redrawn (from the same generator) until the constraints of check_order() hold in both
directions; tests/test_long_lived_cases.py asserts them on the result, so an edit cannot lose
them silently.  order(False) is the forward pass; order(True) runs the units in reverse between
the same first and last unit, which make and destroy the three handles that stay alive through
the whole pass.

A step is a dict: "kind", "size" (elements, pairs or terms: what the call's buffers scale with;
0 for a setting or a destroy call), "cls" (the buffers it shares with other kinds: CLASSES),
its inputs, and "want", the oracle's answer.  step_label() is how a failure names a step."""
import functools

import numpy as np

from oracle import oracle as O
from tests import dev_ordering_cases as D
from tests import msm_basis_cases as B
from tests import msm_g2_cases as C2
from tests import msm_many_cases as M
from tests import msm_prepared_cases as C
from tests.codec_util import compress_g1, compress_g2

SEED = 0x10c9_1fe5_c0de_2026
NT = 16
FRESH = D.FRESH
OK, INVALID, TO_AFFINE = 0, 1, 2
# pairing_many sizes: 1, 7, 33 run k_fe_ds with three blocks per pair on a device of 256 CUs
# (3 n <= CUs), B_PAIRS = 256 // 3 + 1 with one block per pair, 257 is above fe_ds_max (256)
B_PAIRS = 86
# the defaults the setting steps put back (capi.hip)
DEFAULTS = {"fe_wide_max": 8192, "msm_min": 0, "msm_run_max": 0, "msm_window": 0, "msm_many_max": 0,
            "products_wide_max": 8192, "products_min": 8, "fq12_op_unit": 0}
# the buffers a kind's size is measured against: the pairing workspace (and its Fq12 slots), the
# MSM workspaces (integer buffers shared by G1 and G2, the G1 point workspace shared by the
# three G1 forms), the staging area of the host forms
CLASSES = ("pairing", "msm", "stage")
FQ12_OPS = ("mul", "sqr", "inv", "cyc_sqr", "frob1")
GROUP_OPS = ("add", "sub", "neg", "normalize", "eq")
# the groups of kinds that must run next to each other at least once in each direction
ADJACENT = [("pairing_many", "gt_pow_many"), ("g1_msm", "g2_msm"), ("g1_msm", "g1_msm_basis"),
            ("g1_msm", "g1_msm_prepared_many"), ("g1_msm_basis", "g1_msm_prepared_many"),
            ("pairing_batch_many", "pairing_batch_prepared_many"), ("g2_prepare", "pairing_many"),
            ("g1_msm_many:alone", "g1_msm")]
# the kinds with a _dev form that bn254mi.h lists as ordered across streams (the second pass)
DEV_KINDS = ("pairing_many", "pairing_batch", "miller_loop_batch", "pairing_batch_many", "pairing_batch_prepared_many",
             "pairing_prepared_many", "g2_prepare", "g1_msm", "g2_msm", "g1_msm_prepared_many", "g1_msm_many",
             "g1_msm_basis", "g1_bases_prepare", "g1_basis_prepare", "gt_pow_many", "err:prepared_index_dev")


def step_label(s):
    if s is None:
        return "(the start)"
    extra = "".join(" %s=%s" % (k, s[k]) for k in ("route", "name", "handle", "value") if k in s)
    return "%s size %d%s" % (s["kind"], s["size"], extra)


def tagged(s):
    """The kind with its route where the adjacency rules name one."""
    return "%s:%s" % (s["kind"], s["route"]) if s["kind"] == "g1_msm_many" and "route" in s else s["kind"]


def _step(kind, size, cls=None, **kw):
    d = {"kind": kind, "size": int(size), "cls": cls}
    d.update(kw)
    return d


def _set(name, value):
    return _step("set:" + name, 0, name=name, value=value)


def _millers(p, q):
    return np.stack([O.miller_loop_batch(q[k:k + 1], p[k:k + 1])[1] for k in range(p.shape[0])])


def _g1_group(a, b):
    return (O.g1_add(a, b), O.g1_sub(a, b), O.g1_neg(a), O.g1_normalize(a), np.array(O.g1_eq(a, b), np.uint8))


def _g2_group(a, b):
    return (O.g2_add(a, b), O.g2_sub(a, b), O.g2_neg(a), O.g2_normalize(a), np.array(O.g2_eq(a, b), np.uint8))


def _fq12(a, b):
    return {"mul": O.binary("orc_fq12_mul", a, b, 48, 48, 48), "sqr": O.unary("orc_fq12_squared", a, 48)[0],
            "inv": O.unary("orc_fq12_inverse", a, 48)[0], "cyc_sqr": O.unary("orc_fq12_cyclotomic_squared", a, 48)[0],
            "frob1": np.stack([_frob(x, 1) for x in a])}


def _frob(x, pw):
    out = np.zeros(48, np.uint64)
    O.lib().orc_fq12_frobenius_map(O._p(np.ascontiguousarray(x)), pw, O._p(out))
    return out


def _precompute(q):
    out = []
    for k in range(q.shape[0]):
        qa, rc = O.g2_to_affine(q[k])
        assert rc[0] == 0
        out.append(O.g2_precompute(qa[0]))
    return np.stack(out)


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)


class _Pool:
    """The inputs every step slices: 300 G1 points, 257 G2 points, 300 scalars, the 257 pairings
    e(P[i], Q[i]) and the Miller values of the first 128 pairs."""

    def __init__(self):
        self.P = M.g1_points(300, SEED + 1)
        self.Q = C2.g2_points(257, SEED + 2)
        self.k = O.random_scalars(300, seed=SEED + 3, lo=1)[1]
        self.E = O.pairing_many(self.P[:257], self.Q, NT)
        self.ML = _millers(self.P[:128], self.Q[:128])


@functools.lru_cache(maxsize=None)
def pool():
    p = _Pool()
    for a in (p.P, p.Q, p.k, p.E, p.ML):
        a.setflags(write=False)
    return p


# ---- the epoch-wrap tests of tests/test_gpu_long_lived.py
# pairing_batch under bn_set_latency_max(SEG_LATENCY_MAX): at most that many terms run the latency
# product, whose tail has one segment (capi.hip latency_product: cut_plan(1, 1), S = 1, no link
# written); one term more runs the segmented product, whose plan (capi.hip batch_plan) has
# S = 16 segments at every term count up to 34,900.
SEG_LATENCY_MAX = 24
SEG_TERMS = {"S=1": (1, 3, 24), "S=16": (25, 40, 64)}


@functools.lru_cache(maxsize=None)
def seg_tail_products():
    """{(first row, terms): O.pairing_batch of those rows of the pool} for the k_seg_tail test."""
    pl = pool()
    out = {}
    for at, n in ((0, 40), (40, 24), (64, 3), (100, 40), (140, 25), (67, 1), (165, 64), (70, 24), (94, 3), (230, 25)):
        out[(at, n)] = O.pairing_batch(pl.P[at:at + n], pl.Q[at:at + n], NT)
        out[(at, n)].setflags(write=False)
    return out


def _pairs(pool, kind, at, n, **kw):
    """n pairs of the pool from row `at` on: their pairings are rows of pool.E."""
    return _step(kind, n, "pairing", p=pool.P[at:at + n], q=pool.Q[at:at + n], want=pool.E[at:at + n], **kw)


def _products_step(pool, lengths, at, route, routes):
    off = M.offsets_of(lengths)
    n = int(off[-1])
    p, q = pool.P[at:at + n], pool.Q[at:at + n]
    return _step("pairing_batch_many", n, "pairing", p=p, q=q, off=off, route=route, routes=routes,
                 want=D.products(p, q, off))


def _prepared_products_step(pool, handle, table, lengths, at, fresh_every, route, routes):
    off = M.offsets_of(lengths)
    n = int(off[-1])
    p = pool.P[at:at + n]
    qidx = np.array([FRESH if i % fresh_every == 0 else (i * 7 + at) % table.shape[0] for i in range(n)], np.uint32)
    fresh = pool.Q[at:at + int((qidx == FRESH).sum())]
    return _step("pairing_batch_prepared_many", n, "pairing", p=p, q=fresh, handle=handle, qidx=qidx, off=off, route=route,
                 routes=routes, want=D.products(p, D.full_q(qidx, table, fresh), off))


def _churn(pool, at):
    """Seven handles of the three kinds from different points, at most three alive at once (beside
    the three that live through the pass), a freed table's memory handed out again while the
    others are in use: the sequence of tests/test_gpu_long_lived.py run_churn."""
    g2 = [{"q": pool.Q[at + 2 * j:at + 2 * j + 2], "p": pool.P[at + 2 * j:at + 2 * j + 2],
           "want": pool.E[at + 2 * j:at + 2 * j + 2]} for j in range(3)]
    g1p = []
    for j in range(2):
        bases = pool.P[at + 10 + 2 * j:at + 12 + 2 * j]
        scal = np.ascontiguousarray(pool.k[at + 4 * j:at + 4 * j + 4].reshape(2, 2, 4))
        g1p.append({"bases": bases, "scal": scal, "want": C.expect(bases, scal)})
    basis = []
    for j in range(2):
        bases, k = pool.P[at + 20 + 5 * j:at + 25 + 5 * j], pool.k[at + 20 + 5 * j:at + 25 + 5 * j]
        basis.append({"bases": bases, "k": k, "want": B.expect(bases, k)})
    return _step("handle_churn", 7, g2=g2, g1p=g1p, basis=basis)


@functools.lru_cache(maxsize=None)
def script():
    """(first, middle, last): the first unit, the shuffled middle units and the last unit."""
    pl = pool()
    P, Q, K, E, ML = pl.P, pl.Q, pl.k, pl.E, pl.ML[:48]
    zero_g1, zero_g2 = C.zero(), C2.zero()
    # the three handles that live through a pass
    A = Q[200:203]                       # bn_g2_prepare: "A"
    BH = P[260:263]                      # bn_g1_bases_prepare: "Bh"
    CB = P[100:164]                      # bn_g1_basis_prepare: "Cb"
    first = [_step("g2_prepare", 3, "pairing", name="A", q=A),
             _pairs(pl, "pairing_many", 40, 7),
             _step("g1_bases_prepare", 3, "msm", name="Bh", bases=BH),
             _step("g1_basis_prepare", 64, "msm", name="Cb", bases=CB)]
    sc9 = np.ascontiguousarray(K[:27].reshape(9, 3, 4))
    last = [_step("g1_msm_prepared_many", 9, "msm", handle="Bh", scal=sc9, want=C.expect(BH, sc9)),
            _step("g1_prepared_destroy", 0, name="Bh"),
            _step("g1_basis_destroy", 0, name="Cb"),
            _step("err:destroyed_handle", 0, handle="Cb", k=K[:5]),
            _step("g1_msm", 5, "msm", p=P[5:10], k=K[5:10], route="bucket", want=B.expect(P[5:10], K[5:10])),
            _step("g2_prepared_destroy", 0, name="A")]

    units = []
    # Inside a unit most steps follow a step of the same buffers that is larger (L) or smaller (S):
    # with the units' inner order fixed, every sized kind has both relations in either direction
    # whatever the shuffle does (check_order asserts it on the result all the same).
    # ---- pairings: k_fe_ds with three blocks and with one block per pair, above fe_ds_max, and
    # through the throughput kernel; next to gt_pow_many, which reuses their Fq12 slots; the
    # Fq12 operations on both units
    mixed7 = np.concatenate([E[10:13], ML[0:1], E[13:15], ML[1:2]])
    mixed70 = np.concatenate([E[100:131], ML[2:3], E[131:162], ML[3:10]])   # one Miller value inside a Gt wave
    fa, fb = np.concatenate([E[:5], ML[:4]]), np.concatenate([ML[10:14], E[20:25]])
    fa33, fb33 = np.concatenate([E[30:50], ML[20:33]]), np.concatenate([ML[:13], E[50:70]])
    units.append([_pairs(pl, "pairing_many", 0, 257),
                  _set("fq12_op_unit", 1),
                  _step("fq12_op_many", 9, "pairing", a=fa, b=fb, want=_fq12(fa, fb)),                              # L
                  _set("fq12_op_unit", DEFAULTS["fq12_op_unit"]),
                  _step("gt_pow_many", 7, "pairing", a=mixed7, k=K[20:27], want=O.gt_pow(mixed7, K[20:27])),        # L
                  _pairs(pl, "pairing_many", 60, 1),                                                              # L
                  _step("g2_precompute_many", 5, "pairing", q=Q[210:215], want=_precompute(Q[210:215]))])           # S
    units.append([_pairs(pl, "pairing_many", 70, 7),
                  _step("gt_pow_many", 70, "pairing", a=mixed70, k=K[30:100], want=O.gt_pow(mixed70, K[30:100])),   # S
                  _pairs(pl, "pairing_many", 120, 33),
                  _step("g2_precompute_many", 2, "pairing", q=Q[215:217], want=_precompute(Q[215:217]))])           # L
    units.append([_pairs(pl, "pairing_many", 150, B_PAIRS)])
    units.append([_set("fe_wide_max", 0), _pairs(pl, "pairing_many", 3, 33, route="throughput"),
                  _pairs(pl, "pairing_many", 0, 257, route="throughput"),
                  _pairs(pl, "pairing_many", 200, 7, route="throughput"), _set("fe_wide_max", DEFAULTS["fe_wide_max"])])
    # ---- products and Miller loops at 3 and 40 terms
    pb3 = _step("pairing_batch", 3, "pairing", p=P[0:3], q=Q[0:3], want=O.pairing_batch(P[0:3], Q[0:3]))
    pb40 = _step("pairing_batch", 40, "pairing", p=P[50:90], q=Q[50:90], want=O.pairing_batch(P[50:90], Q[50:90]))
    ml3 = _step("miller_loop_batch", 3, "pairing", q=Q[90:93], p=P[90:93], want=O.miller_loop_batch(Q[90:93], P[90:93])[1])
    ml40 = _step("miller_loop_batch", 40, "pairing", q=Q[3:43], p=P[3:43], want=O.miller_loop_batch(Q[3:43], P[3:43])[1])
    units.append([pb3, ml40, pb3])        # S, L
    units.append([ml3, pb40, ml3])        # S, L
    f33 = ML[:33].copy()
    f33[17] = 0
    w33, ok33 = E[:33].copy(), np.ones(33, np.uint8)
    w33[17], ok33[17] = 0, 0
    z48 = np.zeros((1, 48), np.uint64)
    mlm3 = _step("miller_loop_many", 3, "pairing", p=P[44:47], q=Q[44:47], want=ML[44:47])
    fe5 = _step("final_exponentiation_many", 5, "pairing", f=np.concatenate([ML[40:44], z48]),
                want=(np.concatenate([E[40:44], z48]), np.array([1, 1, 1, 1, 0], np.uint8)))
    units.append([mlm3, _step("final_exponentiation_many", 33, "pairing", f=f33, want=(w33, ok33)), mlm3])    # S, L
    units.append([fe5, _step("miller_loop_many", 33, "pairing", p=P[:33], q=Q[:33], want=ML[:33]), fe5])      # S, L
    # ---- prepared G2: a handle of the unit's own next to pairing_many (the pairing workspace), and
    # the long-lived one with and without an index array
    units.append([_pairs(pl, "pairing_many", 61, 1),
                  _step("g2_prepare", 5, "pairing", name="X", q=Q[220:225]),                                        # S
                  _pairs(pl, "pairing_many", 210, 9),                                                             # S
                  _step("pairing_prepared_many", 5, "pairing", p=P[220:225], handle="X", idx=np.arange(5, dtype=np.uint32),
                        want=E[220:225]),                                                                           # L
                  _step("g2_prepared_destroy", 0, name="X"),
                  _step("fq12_op_many", 33, "pairing", a=fa33, b=fb33, want=_fq12(fa33, fb33))])                    # S
    units.append([_pairs(pl, "pairing_many", 100, 65),
                  _step("g2_prepare", 2, "pairing", name="Y", q=Q[230:232]),                                        # L
                  _step("pairing_prepared_many", 2, "pairing", p=P[230:232], handle="Y", idx=np.arange(2, dtype=np.uint32),
                        want=E[230:232]),
                  _step("g2_prepared_destroy", 0, name="Y")])
    i7, i9 = np.array([0, 1, 2, 2, 1, 0, 1], np.uint32), np.array([2, 2, 0, 1, 0, 1, 2, 0, 0], np.uint32)
    want7 = O.pairing_many(P[240:247], A[i7], NT)
    mlp3 = _step("miller_loop_prepared_many", 3, "pairing", p=P[247:250], handle="A", idx=None,
                 want=_millers(P[247:250], np.tile(A[0], (3, 1))))
    units.append([mlp3,
                  _step("pairing_prepared_many", 7, "pairing", p=P[240:247], handle="A", idx=i7, want=want7),       # S
                  _step("miller_loop_prepared_many", 9, "pairing", p=P[250:259], handle="A", idx=i9,
                        want=_millers(P[250:259], A[i9])),                                                          # S
                  _step("pairing_prepared_many", 33, "pairing", p=P[160:193], handle="A", idx=None,
                        want=O.pairing_many(P[160:193], np.tile(A[0], (33, 1)), NT)),
                  mlp3])                                                                                            # L
    # ---- batched products on their three routes, the prepared form wide and packed
    units.append([_products_step(pl, [3, 1, 5, 0, 7, 64, 2, 4, 6], 0, "wide", (9, 0, 0)),
                  _set("products_wide_max", 0),
                  _products_step(pl, [4, 2, 6], 100, "alone", (0, 0, 3)),                                         # L
                  _set("products_min", 0),
                  _products_step(pl, [5, 1, 0, 8, 6], 120, "packed", (0, 5, 0)),                                  # S
                  _prepared_products_step(pl, "A", A, [4, 2, 6, 1, 7, 3], 140, 3, "packed", (0, 6, 0)),           # S
                  _set("products_min", DEFAULTS["products_min"]),
                  _set("products_wide_max", DEFAULTS["products_wide_max"]),
                  _prepared_products_step(pl, "A", A, [2, 9, 4], 170, 4, "wide", (3, 0, 0)),                      # L
                  _products_step(pl, [2, 2], 190, "wide", (2, 0, 0))])
    units.append([_prepared_products_step(pl, "A", A, [1, 3], 30, 2, "wide", (2, 0, 0)),
                  _products_step(pl, [7, 3, 1, 9, 2, 6, 2, 4, 5, 1], 200, "wide", (10, 0, 0))])
    # ---- multiplication
    g2m65 = _step("g2_mul_many", 65, "stage", p=Q[100:165], k=K[100:165], want=O.g2_mul(Q[100:165], K[100:165], NT))
    units.append([_step("g2_mul_many", 9, "stage", p=Q[:9], k=K[:9], want=O.g2_mul(Q[:9], K[:9], NT)),
                  _step("g1_mul_many", 257, "stage", p=P[:257], k=K[:257], want=O.g1_mul(P[:257], K[:257], NT)),    # S
                  g2m65,                                                                                            # L
                  _step("g1_mul_many", 33, "stage", p=P[260:293], k=K[260:293], want=O.g1_mul(P[260:293], K[260:293], NT)),  # L
                  g2m65])                                                                                           # S
    # ---- MSM: the bucket path (the default), the small path, a run cap of one, a window of two;
    # G1 next to G2 (the integer buffers)
    def g1m(at, n, route="bucket"):
        return _step("g1_msm", n, "msm", p=P[at:at + n], k=K[at:at + n], route=route, want=B.expect(P[at:at + n], K[at:at + n]))

    def g2m(at, n, route="bucket"):
        return _step("g2_msm", n, "msm", p=Q[at:at + n], k=K[at:at + n], route=route, want=C2.expect(Q[at:at + n], K[at:at + n]))
    units.append([g1m(0, 300), g2m(0, 65), g1m(40, 40)])                                                            # L, L
    units.append([_set("msm_min", 4096), g1m(7, 33, "small"), g2m(70, 9, "small"), g1m(20, 257, "small"),           # L, S
                  _set("msm_min", DEFAULTS["msm_min"])])
    units.append([_set("msm_run_max", 1), g1m(150, 129), g2m(80, 33), _set("msm_run_max", DEFAULTS["msm_run_max"])])
    units.append([_set("msm_window", 2), g1m(281, 9), g2m(120, 17), g1m(200, 65),                                   # S, S
                  _set("msm_window", DEFAULTS["msm_window"])])
    # ---- the three G1 forms that share the point workspace, pairwise
    sc5 = np.ascontiguousarray(K[100:115].reshape(5, 3, 4))
    sc40 = np.ascontiguousarray(K[120:240].reshape(40, 3, 4))
    sc3 = np.ascontiguousarray(K[240:264].reshape(3, 8, 4))
    units.append([g1m(50, 200),
                  _step("g1_msm_basis", 64, "msm", handle="Cb", k=K[200:264], want=B.expect(CB, K[200:264])),       # L
                  _step("g1_msm_prepared_many", 5, "msm", handle="Bh", scal=sc5, want=C.expect(BH, sc5)),           # L
                  g1m(290, 3)])
    units.append([g1m(293, 3),
                  _step("g1_bases_prepare", 8, "msm", name="W", bases=P[270:278]),                                  # S
                  _step("g1_msm_prepared_many", 3, "msm", handle="W", scal=sc3, want=C.expect(P[270:278], sc3)),
                  _step("g1_msm_basis", 5, "msm", handle="Cb", k=K[270:275], want=B.expect(CB[:5], K[270:275])),    # S
                  _step("g1_msm_prepared_many", 40, "msm", handle="Bh", scal=sc40, want=C.expect(BH, sc40)),        # S
                  _step("g1_prepared_destroy", 0, name="W")])
    # ---- many small MSMs: packed, and with a segment above bn_set_msm_many_max that runs alone
    # on g1_msm's path, next to g1_msm
    l1, l2, l3 = [3, 1, 0, 7, 5, 2], [4, 20, 3], [9, 2, 31, 1, 8, 12, 6]
    o1, o2, o3 = M.offsets_of(l1), M.offsets_of(l2), M.offsets_of(l3)
    units.append([_step("g1_msm_many", 69, "msm", p=P[70:139], k=K[70:139], off=o3, route="packed", want=M.expect(P[70:139], K[70:139], o3)),
                  _step("g1_msm_many", 18, "msm", p=P[10:28], k=K[10:28], off=o1, route="packed", want=M.expect(P[10:28], K[10:28], o1)),  # L
                  _set("msm_many_max", 8),
                  _step("g1_msm_many", 27, "msm", p=P[30:57], k=K[30:57], off=o2, route="alone", want=M.expect(P[30:57], K[30:57], o2)),   # S
                  g1m(60, 7),
                  _set("msm_many_max", DEFAULTS["msm_many_max"])])
    # ---- group law: rows with a == b in another Jacobian scaling, b == -a, and zero operands
    def g1_ops(at, n):
        a, b = P[at:at + n].copy(), P[at + 1:at + n + 1].copy()
        b[0], b[1] = O.g1_normalize(a[0:1])[0], O.g1_neg(a[1:2])[0]
        a[2], b[3] = zero_g1, zero_g1
        return _step("g1_group", n, "stage", a=a, b=b, want=_g1_group(a, b))

    def g2_ops(at, n):
        a, b = Q[at:at + n].copy(), Q[at + 1:at + n + 1].copy()
        b[0], b[1] = O.g2_normalize(a[0:1])[0], O.g2_neg(a[1:2])[0]
        a[2], b[3] = zero_g2, zero_g2
        return _step("g2_group", n, "stage", a=a, b=b, want=_g2_group(a, b))
    g2g65 = g2_ops(100, 65)
    units.append([g2_ops(0, 9), g1_ops(0, 129), g2g65, g1_ops(200, 17), g2g65])                                     # S, L, L, S
    # ---- field and codec
    g = O.SplitMix64(SEED + 4)
    sq = O.canon_to_mont_array([0] + [g.below(O.P) for _ in range(65)]).reshape(-1, 4)
    g2aff, _ = O.g2_to_affine(Q[:33])
    g1aff, _ = O.g1_to_affine(P[:65])
    c1, c2 = compress_g1(g1aff), compress_g2(g2aff)
    c1[5, 0], c2[3, 0] = 4, 12                     # a bad sign byte each
    c1[9, 1:] = np.frombuffer(int(O.P).to_bytes(32, "big"), np.uint8)   # x >= p
    sqrt33 = _step("fq_sqrt_many", 33, "stage", a=sq[:33], want=O.fq_sqrt(sq[:33]))
    g1c9 = _step("g1_from_compressed_many", 9, "stage", b=c1[3:12], want=O.g1_from_compressed(c1[3:12], NT))
    units.append([sqrt33,
                  _step("fq2_sqrt_many", 9, "stage", a=sq[40:58].reshape(9, 8), want=O.fq2_sqrt(sq[40:58].reshape(9, 8))),  # L
                  _step("g1_from_compressed_many", 65, "stage", b=c1, want=O.g1_from_compressed(c1, NT)),                  # S
                  _step("g2_from_compressed_many", 7, "stage", b=c2[:7], want=O.g2_from_compressed(c2[:7], NT))])          # L
    units.append([g1c9,
                  _step("g2_from_compressed_many", 33, "stage", b=c2, want=O.g2_from_compressed(c2, NT)),                  # S
                  _step("fq_sqrt_many", 5, "stage", a=sq[60:65], want=O.fq_sqrt(sq[60:65])),                               # L
                  _step("fq2_sqrt_many", 33, "stage", a=sq.reshape(33, 8), want=O.fq2_sqrt(sq.reshape(33, 8))),            # S
                  g1c9,                                                                                                    # L
                  sqrt33])                                                                                                 # S
    # ---- handle churn
    units.append([_churn(pl, 0)])
    units.append([_churn(pl, 60)])
    units.append([_churn(pl, 130)])
    # ---- outcome steps, each with the call of another kind that runs right behind it
    pz = P[93:96].copy()
    pz[1] = zero_g1
    mlz = _step("err:miller_loop_batch_zero", 3, "pairing", q=Q[93:96], p=pz, code=TO_AFFINE)
    units.append([mlz, _pairs(pl, "pairing_many", 96, 3)])
    units.append([mlz, _step("pairing_batch", 5, "pairing", p=P[110:115], q=Q[110:115], want=O.pairing_batch(P[110:115], Q[110:115]))])
    units.append([_step("err:products_offsets", 6, "pairing", p=P[0:6], q=Q[0:6], off=np.array([0, 4, 2, 6], np.uintp), code=INVALID),
                  _step("miller_loop_batch", 5, "pairing", q=Q[110:115], p=P[110:115], want=O.miller_loop_batch(Q[110:115], P[110:115])[1])])
    units.append([_step("err:products_offsets", 6, "pairing", p=P[0:6], q=Q[0:6], off=np.array([1, 3, 6], np.uintp), code=INVALID),
                  _prepared_products_step(pl, "A", A, [2, 2, 1], 20, 2, "wide", (3, 0, 0))])
    bad7 = i7.copy()
    bad7[3] = 3
    bad_want = want7.copy()
    bad_want[3] = 0
    bad_host = _step("err:prepared_index_host", 7, "pairing", p=P[240:247], handle="A", idx=bad7, code=INVALID)
    bad_dev = _step("err:prepared_index_dev", 7, "pairing", p=P[240:247], handle="A", idx=bad7, want=bad_want, code=INVALID)
    units.append([bad_host, _pairs(pl, "pairing_many", 33, 5)])
    units.append([bad_host, _step("gt_pow_many", 3, "pairing", a=E[5:8], k=K[5:8], want=O.gt_pow(E[5:8], K[5:8]))])
    units.append([bad_dev, _step("pairing_batch", 2, "pairing", p=P[115:117], q=Q[115:117], want=O.pairing_batch(P[115:117], Q[115:117]))])
    units.append([bad_dev, _pairs(pl, "pairing_many", 140, 2)])
    units.append([g1m(280, 9),
                  _step("g1_basis_prepare", 5, "msm", name="Z", bases=P[280:285]),                                  # L
                  _step("g1_msm_basis", 5, "msm", handle="Z", k=K[280:285], want=B.expect(P[280:285], K[280:285])),
                  _step("g1_basis_destroy", 0, name="Z"),
                  _step("err:destroyed_handle", 0, handle="Z", k=K[280:285]),
                  g1m(284, 9)])

    # ---- the order: a seeded shuffle of the units, redrawn until the constraints hold both ways
    rng = O.SplitMix64(SEED)
    for draw in range(1, 2001):
        idx = list(range(len(units)))
        for i in range(len(idx) - 1, 0, -1):      # Fisher-Yates
            j = rng.below(i + 1)
            idx[i], idx[j] = idx[j], idx[i]
        middle = [units[i] for i in idx]
        if not check_order(first, middle, last):
            break
    else:
        raise AssertionError("no order within 2000 draws: " + "; ".join(check_order(first, middle, last)))
    for u in [first, last] + units:
        _freeze(u)
    return first, middle, last, draw


def order(reverse=False):
    """The steps of a pass: the first unit, the middle units (reversed for the second pass), the
    last unit."""
    first, middle, last, _ = script()
    mid = list(reversed(middle)) if reverse else middle
    return list(first) + [s for u in mid for s in u] + list(last)


def _flatten(first, middle, last, reverse):
    mid = list(reversed(middle)) if reverse else middle
    return list(first) + [s for u in mid for s in u] + list(last)


def check_order(first, middle, last):
    """The constraints on the script, in both directions; returns what does not hold."""
    bad = []
    fwd, rev = _flatten(first, middle, last, False), _flatten(first, middle, last, True)
    for name, steps in (("forward", fwd), ("reverse", rev)):
        # the groups of kinds that share a buffer run next to each other at least once
        pairs = {frozenset((tagged(a), tagged(b))) for a, b in zip(steps, steps[1:])}
        pairs |= {frozenset((a["kind"], b["kind"])) for a, b in zip(steps, steps[1:])}
        for x, y in ADJACENT:
            if frozenset((x, y)) not in pairs:
                bad.append("%s: %s and %s never adjacent" % (name, x, y))
        # every outcome step is followed by a call of another kind that runs a kernel
        for a, b in zip(steps, steps[1:] + [None]):
            if a["kind"].startswith("err:") and a["kind"] != "err:destroyed_handle":
                if b is None or b["kind"].startswith(("err:", "set:")) or b["size"] == 0 or "want" not in b:
                    bad.append("%s: nothing checks the outcome word after %s" % (name, a["kind"]))
            if a["kind"] == "err:destroyed_handle" and (b is None or "want" not in b):
                bad.append("%s: nothing runs after %s" % (name, a["kind"]))
        # every setting is back at its default at the end, and handles are used only while alive
        cur, alive = dict(DEFAULTS), set()
        for s in steps:
            if s["kind"].startswith("set:"):
                cur[s["name"]] = s["value"]
            elif s["kind"] in ("g2_prepare", "g1_bases_prepare", "g1_basis_prepare"):
                if s["name"] in alive:
                    bad.append("%s: handle %s made twice" % (name, s["name"]))
                alive.add(s["name"])
            elif s["kind"] in ("g2_prepared_destroy", "g1_prepared_destroy", "g1_basis_destroy"):
                if s["name"] not in alive:
                    bad.append("%s: handle %s destroyed while not alive" % (name, s["name"]))
                alive.discard(s["name"])
            elif "handle" in s and (s["handle"] in alive) == (s["kind"] == "err:destroyed_handle"):
                bad.append("%s: %s with handle %s %s" % (name, s["kind"], s["handle"],
                                                        "alive" if s["handle"] in alive else "not alive"))
        if cur != DEFAULTS:
            bad.append("%s: settings left changed: %s" % (name, {k: v for k, v in cur.items() if v != DEFAULTS[k]}))
        if alive:
            bad.append("%s: handles left alive: %s" % (name, sorted(alive)))
    # Over the context's life (the forward pass, then the reverse pass) every sized kind runs at
    # least once right after a larger call on the buffers it shares and once after a smaller one.
    life = fwd + rev
    seen = {}
    prev = {}
    for s in life:
        if s["cls"] is None or s["size"] == 0 or s["kind"].startswith("err:"):
            continue
        rel = seen.setdefault(s["kind"], {"n": 0, "larger": False, "smaller": False})
        rel["n"] += 1
        p = prev.get(s["cls"])
        if p is not None and p > s["size"]:
            rel["larger"] = True
        if p is not None and p < s["size"]:
            rel["smaller"] = True
        prev[s["cls"]] = s["size"]
    for kind, rel in sorted(seen.items()):
        if rel["n"] < 4:          # twice in each pass
            bad.append("%s runs %d times in two passes" % (kind, rel["n"]))
        if not rel["larger"]:
            bad.append("%s never runs after a larger call on the %s buffers" % (kind, "same"))
        if not rel["smaller"]:
            bad.append("%s never runs after a smaller call on the same buffers" % kind)
    return bad


def handle_counts(steps):
    """(handles made, the most alive at once) over a pass, the churn steps' own included: a churn
    step makes seven and holds at most three beside those alive around it."""
    made = peak = alive = 0
    for s in steps:
        if s["kind"] in ("g2_prepare", "g1_bases_prepare", "g1_basis_prepare"):
            made, alive = made + 1, alive + 1
        elif s["kind"] in ("g2_prepared_destroy", "g1_prepared_destroy", "g1_basis_destroy"):
            alive -= 1
        elif s["kind"] == "handle_churn":
            made += 7
            peak = max(peak, alive + 3)
        peak = max(peak, alive)
    return made, peak


def oracle_pairings():
    """A rough count of the oracle's pairing-sized work behind the script (Miller loops count
    as pairings), for the budget of about 2,000."""
    first, middle, last, _ = script()
    n = 257 + 48
    for s in _flatten(first, middle, last, False):
        if s["kind"] in ("pairing_batch", "miller_loop_batch", "pairing_batch_many", "pairing_batch_prepared_many",
                         "pairing_prepared_many", "miller_loop_prepared_many"):
            n += s["size"]
    return n
