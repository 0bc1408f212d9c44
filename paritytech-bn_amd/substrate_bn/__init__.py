"""substrate_bn -- Python mirror of the substrate-bn 0.6.0 pairing API
(risc0/paritytech-bn src/lib.rs) over the MI355X engine's C ABI.

Same names and argument meaning as the Rust crate for the batched hot path:

    pairing(p: G1, q: G2) -> Gt                        lib.rs:611-613
    pairing_batch([(G1, G2), ...]) -> Gt               lib.rs:615-623
    miller_loop_batch([(G2, G1), ...]) -> Gt           lib.rs:625-633 (raises CurveError)
    Gt.final_exponentiation() -> Gt | None             lib.rs:598-600
    G1 * Fr, G2 * Fr                                   lib.rs:425-431, 575-581
    Gt * Gt                                            lib.rs:603-609

and the wire formats and validation around it:

    Fq.from_slice / to_big_endian / sqrt               lib.rs:154-183
    Fq2.from_slice / sqrt                              lib.rs:238-267
    Fr.from_slice / to_big_endian                      lib.rs:45-55
    AffineG1.new, AffineG2.new (curve + order check)   lib.rs:413-415, 549-551
    G1.from_compressed, G2.from_compressed             lib.rs:359-375, 506-526
    Gt.pow(Fr)                                         lib.rs:592-594

plus the batched forms the reference lacks (pairing_many, g1_mul_many, and the
multi-scalar multiplications g1_msm / g2_msm = sum of points[i] * scalars[i]) that
the engine exists for, and pairings against fixed G2 points prepared once (G2Prepared,
pairing_prepared_many, miller_loop_prepared_many: the reference's G2Precomp held on the
device; pairing_batch_prepared_many: many products whose terms mix fresh and prepared
points), and many small MSMs over fixed G1 bases prepared once (G1Prepared,
g1_msm_prepared_many), and one large MSM per call over a fixed basis prepared once
(G1Basis, g1_msm_basis, g1_msm_basis_many; G2Basis, g2_msm_basis).  Values keep the reference's memory images (canonical
Montgomery, little-endian u64 limbs), so a Gt compares equal exactly when the
reference's derived PartialEq would.  Every computation runs on the GPU; there
is no CPU fallback.
"""
import os

import numpy as np

from . import _native
from ._native import BnError, Context  # noqa: F401

P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
R_ORDER = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
_RM = 1 << 256


class FieldError(Exception):
    """lib.rs:99-104: InvalidSliceLength, InvalidU512Encoding, NotMember (args[0])."""


class CurveError(Exception):
    """lib.rs:106-116: InvalidEncoding, NotMember, Field(FieldError), ToAffineConversion (args[0])."""


class GroupError(Exception):
    """groups/mod.rs:89-92: NotOnCurve, NotInSubgroup (args[0])."""


_FIELD = {1: "InvalidSliceLength", 2: "InvalidU512Encoding", 3: "NotMember"}


def _curve_error(st):
    if st in _FIELD:
        return CurveError("Field", FieldError(_FIELD[st]))
    return CurveError({4: "InvalidEncoding", 5: "NotMember"}[st])


_ctx = None


def context():
    """Process-wide engine context on LOCAL_RANK's device (torch.distributed style)."""
    global _ctx
    if _ctx is None:
        _ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _ctx


def _limbs(x):
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def _int(l):
    return sum(int(v) << (64 * i) for i, v in enumerate(l))


class Fr:
    """Scalar in Montgomery form mod r (fields::Fr, fp.rs:166-193)."""
    __slots__ = ("img",)

    def __init__(self, img):
        self.img = np.ascontiguousarray(img, dtype=np.uint64).reshape(4)

    @classmethod
    def from_int(cls, v):
        return cls(_limbs((v % R_ORDER) * _RM % R_ORDER))

    @classmethod
    def from_str(cls, s):
        """fp.rs:23-43: ASCII decimal digits only (char::to_digit(10)), reduced mod r;
        the empty string is zero; any other character gives None."""
        if not all(c in "0123456789" for c in s):
            return None
        return cls.from_int(int(s, 10) if s else 0)

    @classmethod
    def one(cls):
        return cls.from_int(1)

    @classmethod
    def zero(cls):
        return cls.from_int(0)

    def into_int(self):
        return _int(self.img) * pow(_RM, -1, R_ORDER) % R_ORDER

    def __neg__(self):
        return Fr.from_int(-self.into_int())

    @classmethod
    def from_slice(cls, b):  # lib.rs:45-49: new_mul_factor reduces mod r
        if len(b) != 32:
            raise FieldError("InvalidSliceLength")
        return cls(context().fr_from_slice_many(np.frombuffer(bytes(b), np.uint8))[0])

    def to_big_endian(self):  # lib.rs:50-55: the raw Montgomery image
        return bytes(context().fr_to_big_endian_many(self.img)[0])

    def __eq__(self, o):
        return isinstance(o, Fr) and np.array_equal(self.img, o.img)


class Fq:
    """Base-field element in Montgomery form (fields::Fq, fp.rs:195-222)."""
    __slots__ = ("img",)

    def __init__(self, img):
        self.img = np.ascontiguousarray(img, dtype=np.uint64).reshape(4)

    @classmethod
    def from_int(cls, v):
        return cls(_limbs((v % P) * _RM % P))

    @classmethod
    def from_slice(cls, b):  # lib.rs:154-159
        if len(b) != 32:
            raise FieldError("InvalidSliceLength")
        out, st = context().fq_from_slice_many(np.frombuffer(bytes(b), np.uint8))
        if st[0]:
            raise FieldError(_FIELD[int(st[0])])
        return cls(out[0])

    def to_big_endian(self):  # lib.rs:160-170
        return bytes(context().fq_to_big_endian_many(self.img)[0])

    def sqrt(self):  # fp.rs:245-260
        out, ok = context().fq_sqrt_many(self.img)
        return Fq(out[0]) if ok[0] else None

    def into_int(self):
        return _int(self.img) * pow(_RM, -1, P) % P

    def __eq__(self, o):
        return isinstance(o, Fq) and np.array_equal(self.img, o.img)


class Fq2:
    """c0 + c1 u (fields::Fq2, fq2.rs); img = c0 limbs then c1 limbs."""
    __slots__ = ("img",)

    def __init__(self, img):
        self.img = np.ascontiguousarray(img, dtype=np.uint64).reshape(8)

    @classmethod
    def new(cls, a, b):  # lib.rs:238-240
        return cls(np.concatenate([a.img, b.img]))

    @classmethod
    def from_slice(cls, b):  # lib.rs:260-267
        if len(b) != 64:
            raise FieldError("InvalidU512Encoding")
        out, st = context().fq2_from_slice_many(np.frombuffer(bytes(b), np.uint8))
        if st[0]:
            raise FieldError(_FIELD[int(st[0])])
        return cls(out[0])

    def real(self):
        return Fq(self.img[:4])

    def imaginary(self):
        return Fq(self.img[4:])

    def sqrt(self):  # fq2.rs:208-224
        out, ok = context().fq2_sqrt_many(self.img)
        return Fq2(out[0]) if ok[0] else None

    def __eq__(self, o):
        return isinstance(o, Fq2) and np.array_equal(self.img, o.img)


class _Point:
    WIDTH = 0
    __slots__ = ("img",)

    def __init__(self, img):
        self.img = np.ascontiguousarray(img, dtype=np.uint64).reshape(self.WIDTH)

    def is_zero(self):  # mod.rs:246-248: z == 0
        z = self.img[2 * self.WIDTH // 3:]
        return not z.any()

    def same_image(self, o):
        return type(o) is type(self) and np.array_equal(self.img, o.img)

    # the group law on the engine (bn_{g1,g2}_*_many, lib.rs:388-423, 539-574)
    def _op(self, op, o=None):
        return context().group_op_many(self.GROUP, op, self.img, None if o is None else o.img)

    def __add__(self, o):  # mod.rs:294-334
        return type(self)(self._op("add", o)[0])

    def __sub__(self, o):  # mod.rs:352-358
        return type(self)(self._op("sub", o)[0])

    def __neg__(self):  # mod.rs:336-350
        return type(self)(self._op("neg")[0])

    def normalize(self):  # lib.rs:391-398 (in place, as the reference's &mut self)
        self.img = self._op("normalize")[0]

    def __eq__(self, o):  # PartialEq: projective equality, mod.rs:169-195
        return type(o) is type(self) and bool(self._op("eq", o)[0])

    def __ne__(self, o):
        return not self == o

    __hash__ = None


_MONT_ONE = _limbs(_RM % P)


class G1(_Point):
    """Jacobian G1 point (groups::G1, mod.rs:45-50, 371-402)."""
    WIDTH = 12
    GROUP = "g1"

    @classmethod
    def one(cls):  # mod.rs:381-392: (1, 2, 1)
        return cls(np.concatenate([_MONT_ONE, _limbs(2 * _RM % P), _MONT_ONE]))

    @classmethod
    def zero(cls):  # (0, 1, 0), mod.rs:230-236
        return cls(np.concatenate([np.zeros(4, np.uint64), _MONT_ONE, np.zeros(4, np.uint64)]))

    def __mul__(self, k):
        return G1(context().g1_mul_many(self.img, k.img)[0])

    @classmethod
    def from_compressed(cls, b):  # lib.rs:359-375
        if len(b) != 33:
            raise CurveError("InvalidEncoding")
        out, st = context().g1_from_compressed_many(np.frombuffer(bytes(b), np.uint8))
        if st[0]:
            raise _curve_error(int(st[0]))
        return cls(out[0])

    def x(self):
        return Fq(self.img[0:4])

    def y(self):
        return Fq(self.img[4:8])

    def z(self):
        return Fq(self.img[8:12])


class G2(_Point):
    """Jacobian G2 point over Fq2 (groups::G2, mod.rs:408-472)."""
    WIDTH = 24
    GROUP = "g2"
    _X = (10857046999023057135944570762232829481370756359578518086990519993285655852781,
          11559732032986387107991004021392285783925812861821192530917403151452391805634)
    _Y = (8495653923123431417604973247489272438418190587263600148770280649306958101930,
          4082367875863433681332203403145435568316851327593401208105741076214120093531)

    @classmethod
    def one(cls):  # mod.rs:418-450 (EIP-197 generator), z = 1
        c = [cls._X[0], cls._X[1], cls._Y[0], cls._Y[1], 1, 0]
        return cls(np.concatenate([_limbs(v * _RM % P) for v in c]))

    @classmethod
    def zero(cls):
        z = np.zeros(4, np.uint64)
        return cls(np.concatenate([z, z, _MONT_ONE, z, z, z]))

    def __mul__(self, k):
        return G2(context().g2_mul_many(self.img, k.img)[0])

    @classmethod
    def from_compressed(cls, b):  # lib.rs:506-526
        if len(b) != 65:
            raise CurveError("InvalidEncoding")
        out, st = context().g2_from_compressed_many(np.frombuffer(bytes(b), np.uint8))
        if st[0]:
            raise _curve_error(int(st[0]))
        return cls(out[0])

    def x(self):
        return Fq2(self.img[0:8])

    def y(self):
        return Fq2(self.img[8:16])

    def z(self):
        return Fq2(self.img[16:24])


class AffineG1:
    """lib.rs:397-433; new() validates (mod.rs:95-113, G1: curve equation only)."""

    @staticmethod
    def new(x, y):
        out, st = context().g1_affine_new_many(x.img, y.img)
        if st[0]:
            raise GroupError({6: "NotOnCurve", 7: "NotInSubgroup"}[int(st[0])])
        return G1(out[0])  # From<AffineG1> for G1 (to_jacobian)


class AffineG2:
    """lib.rs:533-571; new() validates the curve equation and the order (mod.rs:95-113)."""

    @staticmethod
    def new(x, y):
        out, st = context().g2_affine_new_many(x.img, y.img)
        if st[0]:
            raise GroupError({6: "NotOnCurve", 7: "NotInSubgroup"}[int(st[0])])
        return G2(out[0])


class Gt:
    """Target group element (Gt(Fq12), lib.rs:584-609)."""
    __slots__ = ("img",)

    def __init__(self, img):
        self.img = np.ascontiguousarray(img, dtype=np.uint64).reshape(48)

    @classmethod
    def one(cls):
        img = np.zeros(48, np.uint64)
        img[:4] = _MONT_ONE
        return cls(img)

    def __mul__(self, o):
        return Gt(context().fq12_op_many("mul", self.img, o.img)[0])

    def pow(self, k):  # lib.rs:592-594
        return Gt(context().gt_pow_many(self.img, k.img)[0])

    def final_exponentiation(self):
        out, ok = context().final_exponentiation_many(self.img)
        return Gt(out[0]) if ok[0] else None

    def __eq__(self, o):
        return isinstance(o, Gt) and np.array_equal(self.img, o.img)

    def __ne__(self, o):
        return not self.__eq__(o)

    def __repr__(self):
        return "Gt(%s)" % ", ".join("%x" % _int(self.img[4 * k:4 * k + 4]) for k in range(12))


def pairing(p, q):
    return Gt(context().pairing_many(p.img, q.img)[0])


def pairing_batch(pairs):
    pairs = list(pairs)
    p = np.stack([a.img for a, _ in pairs]) if pairs else np.zeros((0, 12), np.uint64)
    q = np.stack([b.img for _, b in pairs]) if pairs else np.zeros((0, 24), np.uint64)
    return Gt(context().pairing_batch(p, q))


def pairing_batch_many(products):
    """[pairing_batch(pairs) for pairs in products] in one engine call (bn_pairing_batch_many).
    products: a sequence of sequences of (G1, G2); an empty product gives Gt.one(); no
    products give [] without a device call."""
    products = [list(pairs) for pairs in products]
    if not products:
        return []
    offsets = np.zeros(len(products) + 1, np.uintp)
    offsets[1:] = np.cumsum([len(pairs) for pairs in products])
    flat = [pair for pairs in products for pair in pairs]
    p = np.stack([a.img for a, _ in flat]) if flat else np.zeros((0, 12), np.uint64)
    q = np.stack([b.img for _, b in flat]) if flat else np.zeros((0, 24), np.uint64)
    return [Gt(row) for row in context().pairing_batch_many(p, q, offsets)]


def miller_loop_batch(pairs):
    pairs = list(pairs)
    q = np.stack([a.img for a, _ in pairs]) if pairs else np.zeros((0, 24), np.uint64)
    p = np.stack([b.img for _, b in pairs]) if pairs else np.zeros((0, 12), np.uint64)
    try:
        return Gt(context().miller_loop_batch(q, p))
    except BnError as e:
        if e.code == _native.BN_ERR_TO_AFFINE:
            raise CurveError("ToAffineConversion") from None
        raise


# ---- batched forms (numpy arrays of memory images)
def pairing_many(p, q):
    return context().pairing_many(p, q)


def g1_mul_many(p, k):
    return context().g1_mul_many(p, k)


def g2_mul_many(p, k):
    return context().g2_mul_many(p, k)


def _images(xs, width):
    """(n, width) uint64 rows from a sequence of G1 / G2 / Fr values or an array of images."""
    if isinstance(xs, np.ndarray):
        return _native._arr(xs, width)
    xs = list(xs)
    if not xs:
        return np.zeros((0, width), np.uint64)
    return np.stack([np.asarray(getattr(x, "img", x), dtype=np.uint64).reshape(width) for x in xs])


def g1_msm(points, scalars):
    """sum of points[i] * scalars[i] as a normalized G1 (bn_g1_msm).  Takes sequences of
    G1 / Fr or the (n, 12) / (n, 4) image arrays; no terms give G1.zero() without a
    device call; different lengths raise ValueError."""
    p, k = _images(points, 12), _images(scalars, 4)
    if p.shape[0] != k.shape[0]:
        raise ValueError("g1_msm: %d points and %d scalars" % (p.shape[0], k.shape[0]))
    if p.shape[0] == 0:
        return G1.zero()
    return G1(context().g1_msm(p, k))


def g1_msm_many(msms, ctx=None):
    """[g1_msm(points, scalars) for points, scalars in msms] in one engine call
    (bn_g1_msm_many): many small MSMs over fresh bases, as a batch of PLONK / KZG verifiers
    computes them.  msms: a sequence of (points, scalars), each as g1_msm takes them; an MSM
    of no terms gives G1.zero(); different lengths in one of them raise ValueError before any
    device call; no MSMs give [] without one."""
    parts = []
    for points, scalars in msms:
        p, k = _images(points, 12), _images(scalars, 4)
        if p.shape[0] != k.shape[0]:
            raise ValueError("g1_msm_many: %d points and %d scalars in MSM %d" % (p.shape[0], k.shape[0], len(parts)))
        parts.append((p, k))
    if not parts:
        return []
    offsets = np.zeros(len(parts) + 1, np.uintp)
    offsets[1:] = np.cumsum([p.shape[0] for p, _ in parts])
    p = np.concatenate([p for p, _ in parts])
    k = np.concatenate([k for _, k in parts])
    return [G1(row) for row in (ctx or context()).g1_msm_many(p, k, offsets)]


def g2_msm(points, scalars):
    """sum of points[i] * scalars[i] as a normalized G2 (bn_g2_msm).  Takes sequences of
    G2 / Fr or the (n, 24) / (n, 4) image arrays; no terms give G2.zero() without a
    device call; different lengths raise ValueError."""
    p, k = _images(points, 24), _images(scalars, 4)
    if p.shape[0] != k.shape[0]:
        raise ValueError("g2_msm: %d points and %d scalars" % (p.shape[0], k.shape[0]))
    if p.shape[0] == 0:
        return G2.zero()
    return G2(context().g2_msm(p, k))


class G2Prepared:
    """The line coefficients of fixed G2 points held on the device (bn_g2_prepare; the
    reference's G2Precomp, mod.rs:566-577, per point): what a verifier builds once from its
    verifying key, SRS element or public keys and then pairs many G1 points against
    (pairing_prepared_many, miller_loop_prepared_many).  Built from a sequence of G2 (or an
    (n, 24) image array), 1 .. 65536 of them; zero points are allowed.  len() is the number
    of points.  Release it with close(), a `with` block, or by dropping it; it belongs to
    the engine context it was built on (the process-wide one unless `ctx` is given)."""

    def __init__(self, points, ctx=None):
        self._h = None
        q = _images(points, 24)
        if not 1 <= q.shape[0] <= 1 << 16:
            raise ValueError("G2Prepared takes 1 .. 65536 points, not %d" % q.shape[0])
        self._ctx = ctx if ctx is not None else context()
        self._n = q.shape[0]
        self._h = self._ctx.g2_prepare(q)

    def __len__(self):
        return self._n

    @property
    def closed(self):
        return self._h is None

    def _handle(self):
        if self._h is None:
            raise ValueError("this G2Prepared is closed")
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        # (a context closed first has freed its handles itself)
        if h is not None and getattr(self._ctx, "handle", None):
            self._ctx.g2_prepared_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _prepared_rows(method, ps, prepared, idx):
    p = _images(ps, 12)
    h = prepared._handle()
    if p.shape[0] == 0:
        return []
    ix = _native._indices(idx if idx is None or isinstance(idx, np.ndarray) else list(idx), p.shape[0], len(prepared))
    return [Gt(row) for row in getattr(prepared._ctx, method)(p, h, ix)]


def pairing_prepared_many(ps, prepared, idx=None):
    """[pairing(ps[i], prepared[idx[i]])] in one engine call (bn_pairing_prepared_many), the same
    Gt as pairing() on each pair.  ps: a sequence of G1 or an (n, 12) image array; idx: one
    index per pair, or None for prepared point 0 throughout.  An index outside the prepared
    points, a negative one and a closed G2Prepared raise ValueError before any device call;
    no pairs give []."""
    return _prepared_rows("pairing_prepared_many", ps, prepared, idx)


def miller_loop_prepared_many(ps, prepared, idx=None):
    """The Miller values of the same pairs (G2Precomp::miller_loop at ps[i].to_affine(),
    mod.rs:579-607) as Gt-shaped values, before any final exponentiation
    (bn_miller_loop_prepared_many).  Arguments as pairing_prepared_many."""
    return _prepared_rows("miller_loop_prepared_many", ps, prepared, idx)


def pairing_batch_prepared_many(products, prepared):
    """[pairing_batch(pairs) for pairs in products] in one engine call
    (bn_pairing_batch_prepared_many) where a term's G2 side may be a prepared point: each
    term is (G1, G2), a fresh point, or (G1, int), index into `prepared` (a G2Prepared),
    whose line steps are then not recomputed.  The same Gt as pairing_batch with the points
    written out.  An index outside the prepared points, a product of more than 64 terms and
    a closed G2Prepared raise ValueError before any device call; an empty product gives
    Gt.one(); no products give [] without a device call."""
    products = [list(terms) for terms in products]
    h = prepared._handle()
    nq = len(prepared)
    for terms in products:
        if len(terms) > _native.PRODUCT_LANE_MAX:
            raise ValueError("a product of %d terms (at most %d); use pairing_batch"
                             % (len(terms), _native.PRODUCT_LANE_MAX))
        for _, b in terms:
            if isinstance(b, (int, np.integer)) and not 0 <= int(b) < nq:
                raise ValueError("prepared-point index %d outside 0 .. %d" % (int(b), nq - 1))
    if not products:
        return []
    offsets = np.zeros(len(products) + 1, np.uintp)
    offsets[1:] = np.cumsum([len(terms) for terms in products])
    flat = [term for terms in products for term in terms]
    fresh = [b for _, b in flat if not isinstance(b, (int, np.integer))]
    qidx = np.array([int(b) if isinstance(b, (int, np.integer)) else _native.QIDX_FRESH for _, b in flat], np.uint32)
    p = np.stack([a.img for a, _ in flat]) if flat else np.zeros((0, 12), np.uint64)
    q = np.stack([b.img for b in fresh]) if fresh else np.zeros((0, 24), np.uint64)
    return [Gt(row) for row in prepared._ctx.pairing_batch_prepared_many(p, q, h, qidx, offsets)]


class G1Prepared:
    """Window tables of fixed G1 bases held on the device (bn_g1_bases_prepare): what a
    verifier builds once from its verifying key's IC points, or a committer from its basis,
    and then runs many small MSMs over (g1_msm_prepared_many).  Built from a sequence of G1
    (or a (k, 12) image array) of at least one base; zero bases are allowed.  `window` is
    the table's width in bits, 2 .. 16 (0: the engine's default); len() is the number of
    bases.  Release it with close(), a `with` block, or by dropping it; it belongs to the
    engine context it was built on (the process-wide one unless `ctx` is given)."""

    def __init__(self, bases, window=0, ctx=None):
        self._h = None
        b = _images(bases, 12)
        if b.shape[0] < 1:
            raise ValueError("G1Prepared takes at least one base")
        if window != 0 and not 2 <= window <= 16:
            raise ValueError("G1Prepared window must be 0 or 2 .. 16, not %r" % (window,))
        self._ctx = ctx if ctx is not None else context()
        self._n = b.shape[0]
        self._h = self._ctx.g1_bases_prepare(b, window)
        self.window = self._ctx.g1_prepared_window(self._h)

    def __len__(self):
        return self._n

    @property
    def closed(self):
        return self._h is None

    def _handle(self):
        if self._h is None:
            raise ValueError("this G1Prepared is closed")
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        # (a context closed first has freed its handles itself)
        if h is not None and getattr(self._ctx, "handle", None):
            self._ctx.g1_prepared_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def g1_msm_prepared_many(prepared, rows):
    """[sum_b prepared[b] * row[b] for row in rows] as normalized G1 in one engine call
    (bn_g1_msm_prepared_many), each the same G1 as g1_msm over the bases and that row.  rows:
    a sequence of sequences of Fr, one scalar per base, or an (m, k, 4) image array.  A row
    whose length is not len(prepared) and a closed G1Prepared raise ValueError before any
    device call; no rows give []."""
    h = prepared._handle()
    k = len(prepared)
    if isinstance(rows, np.ndarray):
        s = np.ascontiguousarray(rows, dtype=np.uint64)
        if s.ndim != 3 or s.shape[1:] != (k, 4):
            raise ValueError("g1_msm_prepared_many: scalars of shape %s are not rows of %d Fr" % (s.shape, k))
    else:
        rows = [list(r) for r in rows]
        for r in rows:
            if len(r) != k:
                raise ValueError("g1_msm_prepared_many: a row of %d scalars for %d bases" % (len(r), k))
        s = _images([x for r in rows for x in r], 4).reshape(len(rows), k, 4)
    if s.shape[0] == 0:
        return []
    return [G1(row) for row in prepared._ctx.g1_msm_prepared_many(h, s)]


class _Basis:
    """What G1Basis and G2Basis share: the argument checks, the handle's lifetime and the
    `with` protocol.  A subclass names the words of a base's image and its five engine calls."""

    _WORDS = 0

    def _prepare(self, b, window):
        raise NotImplementedError

    def _prepare_dev(self, address, count, window, stream):
        raise NotImplementedError

    def _count(self, h):
        raise NotImplementedError

    def _window(self, h):
        raise NotImplementedError

    def _destroy(self, h):
        raise NotImplementedError

    def __init__(self, bases, window=0, ctx=None, count=None, stream=None):
        self._h = None
        name = type(self).__name__
        if window != 0 and not 2 <= window <= 16:
            raise ValueError("%s window must be 0 or 2 .. 16, not %r" % (name, window))
        if isinstance(bases, int):
            if count is None or count < 1:
                raise ValueError("%s from a device address takes count >= 1" % name)
            self._ctx = ctx if ctx is not None else context()
            self._h = self._prepare_dev(bases, count, window, stream)
        else:
            b = _images(bases, self._WORDS)
            if b.shape[0] < 1:
                raise ValueError("%s takes at least one base" % name)
            if count is not None and count != b.shape[0]:
                raise ValueError("%s: count %d for %d bases" % (name, count, b.shape[0]))
            self._ctx = ctx if ctx is not None else context()
            self._h = self._prepare(b, window)
        self.count = self._count(self._h)
        self.window = self._window(self._h)

    def __len__(self):
        return self.count

    @property
    def closed(self):
        return self._h is None

    def _handle(self):
        if self._h is None:
            raise ValueError("this %s is closed" % type(self).__name__)
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        # (a context closed first has freed its handles itself)
        if h is not None and getattr(self._ctx, "handle", None):
            self._destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class G1Basis(_Basis):
    """A fixed G1 basis held on the device for large MSMs (bn_g1_basis_prepare): what a
    committer builds once from its SRS, or a prover from its proving key's queries, and then
    runs one MSM per call over (g1_msm_basis).  For every base and every window of the
    recoding it holds the one point 2^(window * w) * base, so a call adds table points into
    buckets and doubles nothing.  Built from a sequence of G1 or a (n, 12) image array of at
    least one base, or from a device address (`bases` an int, `count` the number of bases, on
    `stream`); zero bases are allowed.  `window` is the width in bits, 2 .. 16 (0: the engine's
    default for that many bases); len() and `count` are the number of bases.  Release it with
    close(), a `with` block, or by dropping it; it belongs to the engine context it was built
    on (the process-wide one unless `ctx` is given)."""

    _WORDS = 12

    def _prepare(self, b, window):
        return self._ctx.g1_basis_prepare(b, window)

    def _prepare_dev(self, address, count, window, stream):
        return self._ctx.g1_basis_prepare_dev(address, count, window, stream)

    def _count(self, h):
        return self._ctx.g1_basis_count(h)

    def _window(self, h):
        return self._ctx.g1_basis_window(h)

    def _destroy(self, h):
        self._ctx.g1_basis_destroy(h)


def g1_msm_basis(basis, scalars):
    """sum of basis[i] * scalars[i] over the first len(scalars) bases as a normalized G1
    (bn_g1_msm_basis), the same G1 as g1_msm over those bases.  scalars: a sequence of Fr or an
    (n, 4) image array.  More scalars than bases and a closed G1Basis raise ValueError before
    any device call; no scalars give G1.zero() without one."""
    h = basis._handle()
    k = _images(scalars, 4)
    if k.shape[0] > len(basis):
        raise ValueError("g1_msm_basis: %d scalars for a basis of %d" % (k.shape[0], len(basis)))
    if k.shape[0] == 0:
        return G1.zero()
    return G1(basis._ctx.g1_msm_basis(h, k))


def g1_msm_basis_many(basis, scalars_2d):
    """One MSM per row of scalars_2d over the first (row length) bases of the G1Basis, in one
    call (bn_g1_msm_basis_many): an (m, 12) array whose row j is the image g1_msm_basis returns
    for row j.  scalars_2d: a sequence of m equally long sequences of Fr, or an (m, n, 4) image
    array.  Rows longer than the basis, ragged rows and a closed G1Basis raise ValueError
    before any device call; no rows give an empty (0, 12) array without one."""
    h = basis._handle()
    if isinstance(scalars_2d, np.ndarray):
        k = np.ascontiguousarray(scalars_2d, dtype=np.uint64)
    else:
        rows = [_images(r, 4) for r in scalars_2d]
        if len({r.shape[0] for r in rows}) > 1:
            raise ValueError("g1_msm_basis_many: rows of different lengths")
        k = np.stack(rows) if rows else np.zeros((0, 0, 4), np.uint64)
    if k.ndim != 3 or k.shape[2] != 4:
        raise ValueError("g1_msm_basis_many: scalars of shape %s are not rows of Fr images" % (k.shape,))
    if k.shape[1] > len(basis):
        raise ValueError("g1_msm_basis_many: %d scalars per row for a basis of %d" % (k.shape[1], len(basis)))
    if k.shape[0] == 0:
        return np.zeros((0, 12), np.uint64)
    return basis._ctx.g1_msm_basis_many(h, k)


class G2Basis(_Basis):
    """A fixed G2 basis held on the device for large MSMs (bn_g2_basis_prepare): a Groth16
    prover's B query, the G2 powers of tau of an SRS.  As G1Basis in every respect, over G2
    or (n, 24) image arrays; run MSMs over it with g2_msm_basis."""

    _WORDS = 24

    def _prepare(self, b, window):
        return self._ctx.g2_basis_prepare(b, window)

    def _prepare_dev(self, address, count, window, stream):
        return self._ctx.g2_basis_prepare_dev(address, count, window, stream)

    def _count(self, h):
        return self._ctx.g2_basis_count(h)

    def _window(self, h):
        return self._ctx.g2_basis_window(h)

    def _destroy(self, h):
        self._ctx.g2_basis_destroy(h)


def g2_msm_basis(basis, scalars):
    """sum of basis[i] * scalars[i] over the first len(scalars) bases as a normalized G2
    (bn_g2_msm_basis), the same G2 as g2_msm over those bases.  scalars: a sequence of Fr or an
    (n, 4) image array.  More scalars than bases and a closed G2Basis raise ValueError before
    any device call; no scalars give G2.zero() without one."""
    h = basis._handle()
    k = _images(scalars, 4)
    if k.shape[0] > len(basis):
        raise ValueError("g2_msm_basis: %d scalars for a basis of %d" % (k.shape[0], len(basis)))
    if k.shape[0] == 0:
        return G2.zero()
    return G2(basis._ctx.g2_msm_basis(h, k))


def g2_affine_new_many(x, y):
    """(G2 images, bn_elem_status) for arrays of affine (x, y): AffineG2::new batched."""
    return context().g2_affine_new_many(x, y)


def g1_from_compressed_many(b33):
    return context().g1_from_compressed_many(b33)


def g2_from_compressed_many(b65):
    return context().g2_from_compressed_many(b65)


def gt_pow_many(a, k):
    return context().gt_pow_many(a, k)
