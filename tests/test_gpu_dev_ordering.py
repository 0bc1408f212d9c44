"""The device-pointer (_dev) calls' promises across caller streams (include/bn254mi.h):

1. _dev calls that use a context workspace or read a handle run on the device in call order,
   whatever streams they are enqueued on (ws_event, capi_internal.h), and the pinned control
   arrays of one call are not rewritten before the previous call's upload has read them;
2. the calls documented to wait (bn_dev_status, the destroy calls, a call that regrows a
   workspace) return only when the queued work is done;
3. the status-less calls leave a sticky outcome that bn_dev_status reports, also when a call
   with a status word of its own runs in between.

How a missing order is made visible.  Call A goes on stream s1 behind a device-side delay;
call B goes on another stream and reads A's output buffer, which holds a valid placeholder V0
(the generator, Gt::one(); tests/dev_ordering_cases.py) until A writes it.  An event e0 sits on
s1 between the delay and A: `not e0.query()` after the last call has returned shows that every
call was enqueued before A could begin, so nothing but the library orders B after A.  A B that
ran early would return the oracle's answer for V0, which differs from the expected value in
every dependent row (tests/test_dev_ordering_cases.py).  If e0 has completed (a slow host), the
sequence is repeated with the delay doubled, three attempts in all, and then fails.  Each call
of a sequence runs once beforehand with host synchronization: that checks its result alone and
sizes every buffer, so that no call of the sequence allocates (an allocating call waits for
earlier work, which would hide a missing order).  test_harness_sees_a_missing_order shows that
the rig does see one.

Delay that satisfied the e0 condition on the MI355X: 20 ms, the first attempt, for every chain
and sequence below (each prints the delay it needed)."""
import numpy as np
import pytest

from tests import dev_ordering_cases as D

pytestmark = pytest.mark.gpu
DELAYS_MS = (20, 40, 80)
OK, INVALID = 0, 1


# ---------------------------------------------------------------- the rig
class Rig:
    """Three caller streams with s2 and s3 free to run while s1 is held, a calibrated
    device-side delay, and the upload / read-back helpers."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.s1 = torch.cuda.Stream(self.dev)
        self._scratch = torch.zeros(64, dtype=torch.int64, device=self.dev)
        self._calibrate()
        # caller streams may share a hardware queue, which would order them by itself: keep
        # only streams whose work completes while s1 is held
        free = []
        for _ in range(8):
            s = torch.cuda.Stream(self.dev)
            if self._runs_beside_s1(s):
                free.append(s)
            if len(free) == 2:
                break
        assert len(free) == 2, "no two streams run while another stream is held: the rig cannot see a missing order"
        self.s2, self.s3 = free

    def _calibrate(self):
        torch = self.torch
        if hasattr(torch.cuda, "_sleep"):
            cycles = 2_000_000  # 1 ms at a 2 GHz counter, 20 ms at a 100 MHz one
            torch.cuda._sleep(1000)
            torch.cuda.synchronize(self.dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            self._per_ms = max(1.0, cycles / max(a.elapsed_time(b), 1e-3))
            self._mat = None
        else:  # a run of large matrix products instead
            self._mat = torch.randn(4096, 4096, device=self.dev)
            torch.mm(self._mat, self._mat)
            torch.cuda.synchronize(self.dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(4):
                torch.mm(self._mat, self._mat)
            b.record()
            b.synchronize()
            self._per_ms = max(1e-3, 4 / max(a.elapsed_time(b), 1e-3))

    def hold(self, ms):
        """`ms` of device-side delay on s1, then an event: complete once the delay is over."""
        torch = self.torch
        with torch.cuda.stream(self.s1):
            if self._mat is None:
                torch.cuda._sleep(int(ms * self._per_ms))
            else:
                for _ in range(int(ms * self._per_ms) + 1):
                    torch.mm(self._mat, self._mat)
            e0 = torch.cuda.Event()
            e0.record()
        return e0

    def _runs_beside_s1(self, s):
        torch = self.torch
        e0 = self.hold(DELAYS_MS[0])
        with torch.cuda.stream(s):
            self._scratch.add_(1)
            e = torch.cuda.Event()
            e.record()
        e.synchronize()
        beside = not e0.query()
        torch.cuda.synchronize(self.dev)
        return beside

    def event(self, stream):
        e = self.torch.cuda.Event()
        e.record(stream)
        return e

    def sync(self):
        self.torch.cuda.synchronize(self.dev)

    def up(self, a, dtype=np.uint64):
        a = np.ascontiguousarray(a, dtype=dtype)
        view = {np.uint64: np.int64, np.uint32: np.int32}[dtype]
        t = self.torch.from_numpy(a.view(view).reshape(-1).copy()).to(self.dev)
        self.sync()
        return t

    def zeros(self, words):
        t = self.torch.zeros(words, dtype=self.torch.int64, device=self.dev)
        self.sync()
        return t

    @staticmethod
    def rows(t, width):
        return t.cpu().numpy().view(np.uint64).reshape(-1, width)


@pytest.fixture(scope="module")
def rig():
    return Rig()


@pytest.fixture(scope="module")
def cases():
    return D.cases()


@pytest.fixture
def ctx():
    """A context of its own for every test: the tests change settings and grow workspaces."""
    from substrate_bn import Context
    c = Context(0)
    yield c
    c.close()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, "%s: rows %s differ" % (what, bad[:8].tolist())


def warm(rig, reset, steps):
    """Every call once with host synchronization, each result checked alone."""
    reset()
    rig.sync()
    for call, verify in steps:
        call()
        rig.sync()
        if verify:
            verify()


def ordered(rig, label, reset, steps, assert_e0=True):
    """The calls of `steps` back to back behind a delay on s1, then every check.  Returns the
    delay at which all calls were enqueued before the first could begin."""
    warm(rig, reset, steps)
    for ms in DELAYS_MS:
        reset()
        rig.sync()
        e0 = rig.hold(ms)
        for call, _ in steps:
            call()
        enqueued_first = not e0.query()
        rig.sync()
        for _, verify in steps:
            if verify:
                verify()
        print("%s: delay %d ms, every call enqueued before the first could begin: %s" % (label, ms, enqueued_first))
        if enqueued_first or not assert_e0:
            return ms
    raise AssertionError("%s: the calls did not return within %d ms of device delay" % (label, DELAYS_MS[-1]))


def test_harness_sees_a_missing_order(rig, cases):
    """The producer is a plain copy of the right value on s1 behind the delay and nothing orders
    s2 after it: the consumer, a library call on s2, must return the V0 answer.  A context of
    its own, whose only earlier call has long completed, so ws_event plays no part."""
    from substrate_bn import Context
    c = cases["msm_pairs"]
    ctx = Context(0)
    try:
        P3, Q3, out = rig.up(c["p3_v0"]), rig.up(c["q3"]), rig.zeros(3 * 48)
        v0, right = rig.up(c["p3_v0"]), rig.up(c["sum"])
        consume = lambda: ctx.pairing_many_dev(P3.data_ptr(), Q3.data_ptr(), 3, out.data_ptr(), rig.s2.cuda_stream)  # noqa: E731
        consume()
        rig.sync()
        same(rig.rows(out, 48), c["v0_many"], "the consumer alone")
        for ms in DELAYS_MS:
            P3.copy_(v0)
            out.zero_()
            rig.sync()
            e0 = rig.hold(ms)
            with rig.torch.cuda.stream(rig.s1):
                P3[:12].copy_(right)
            consume()
            early = not e0.query()
            rig.sync()
            print("harness self-check: delay %d ms, consumer enqueued before the producer could begin: %s" % (ms, early))
            if early:
                break
        assert early
        same(rig.rows(out, 48), c["v0_many"], "an unordered consumer reads V0")
        same(rig.rows(P3, 12), c["p3"], "the producer ran afterwards")
    finally:
        ctx.close()


# ---------------------------------------------------------------- chains: A on s1, B on s2
def test_msm_many_then_prepared_products(rig, cases, ctx):
    """The header's PLONK flow: the segment sums written into every second slot of the
    products' p array.  Delay needed: 20 ms."""
    c = cases["many_products"]
    ctx.g1_msm_many_reserve(15, 5)
    ctx.reserve(16)
    h = ctx.g2_prepare(c["table"])
    try:
        P, K, PAIRS, V0 = rig.up(c["p"]), rig.up(c["k"]), rig.up(c["pairs_v0"]), rig.up(c["pairs_v0"])
        gt = rig.zeros(5 * 48)
        steps = [
            (lambda: ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), c["off"], PAIRS.data_ptr(), 2, rig.s1.cuda_stream),
             lambda: same(rig.rows(PAIRS, 12), c["pairs"], "the sums in the p array")),
            (lambda: ctx.pairing_batch_prepared_many_dev(PAIRS.data_ptr(), None, h, c["qidx"], c["poff"], gt.data_ptr(),
                                                         rig.s2.cuda_stream),
             lambda: same(rig.rows(gt, 48), c["want"], "the products"))]
        ordered(rig, "msm_many -> prepared products", lambda: (PAIRS.copy_(V0), gt.zero_()), steps)
        ctx.dev_status()
    finally:
        ctx.g2_prepared_destroy(h)


@pytest.mark.parametrize("path", ["wide", "packed"])
def test_msm_prepared_then_prepared_products(rig, cases, ctx, path):
    """Groth16: vk_x at stride 4 straight into the interleaved p array, then the products on the
    wide path and, with the wide path off, on the packed one.  Delay needed: 20 ms on both."""
    c = cases["prepared_products"]
    if path == "packed":
        ctx.set_products_wide_max(0)
    ctx.msm_reserve(5 * 64)
    ctx.reserve(32)
    g1h = ctx.g1_bases_prepare(c["bases"])
    g2h = ctx.g2_prepare(c["table"])
    try:
        K, PAIRS, V0, QF = rig.up(c["scal"]), rig.up(c["pairs_v0"]), rig.up(c["pairs_v0"]), rig.up(c["fresh"])
        gt = rig.zeros(5 * 48)
        steps = [
            (lambda: ctx.g1_msm_prepared_many_dev(g1h, K.data_ptr(), 5, PAIRS.data_ptr(), 4, rig.s1.cuda_stream),
             lambda: same(rig.rows(PAIRS, 12), c["pairs"], "vk_x in the p array")),
            (lambda: ctx.pairing_batch_prepared_many_dev(PAIRS.data_ptr(), QF.data_ptr(), g2h, c["qidx"], c["poff"],
                                                         gt.data_ptr(), rig.s2.cuda_stream),
             lambda: same(rig.rows(gt, 48), c["want"], "the products"))]
        ctx.products_routes()
        ordered(rig, "msm_prepared -> prepared products (%s)" % path, lambda: (PAIRS.copy_(V0), gt.zero_()), steps)
        wide, packed, alone = ctx.products_routes()
        assert alone == 0 and (packed == 0 if path == "wide" else wide == 0) and wide + packed > 0
        ctx.dev_status()
    finally:
        ctx.g1_prepared_destroy(g1h)
        ctx.g2_prepared_destroy(g2h)


def test_msm_then_pairing_batch(rig, cases, ctx):
    """The bucket path (bn_set_msm_min(0)) at 257 terms, its sum as p[0] of a three-pair
    product with a status word.  Delay needed: 20 ms."""
    c = cases["msm_pairs"]
    ctx.set_msm_min(0)
    ctx.msm_reserve(257)
    ctx.reserve(3)
    P, K, P3, V0, Q3 = rig.up(c["p"]), rig.up(c["k"]), rig.up(c["p3_v0"]), rig.up(c["p3_v0"]), rig.up(c["q3"])
    gt = rig.zeros(48)
    st = rig.torch.full((1,), -1, dtype=rig.torch.int32, device=rig.dev)

    def check_b():
        assert int(st.item()) == OK
        same(rig.rows(gt, 48), c["want_batch"][None, :], "the product")
    steps = [
        (lambda: ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), 257, P3.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(P3, 12), c["p3"], "the sum as p[0]")),
        (lambda: ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, gt.data_ptr(), st.data_ptr(), rig.s2.cuda_stream),
         check_b)]
    ordered(rig, "g1_msm -> pairing_batch", lambda: (P3.copy_(V0), gt.zero_(), st.fill_(-1)), steps)


def test_msm_basis_then_pairing_many(rig, cases, ctx):
    """Delay needed: 20 ms."""
    c = cases["msm_pairs"]
    h = ctx.g1_basis_prepare(c["p"])
    try:
        ctx.g1_msm_basis_reserve(h, 257)
        ctx.reserve(3)
        K, P3, V0, Q3 = rig.up(c["k"]), rig.up(c["p3_v0"]), rig.up(c["p3_v0"]), rig.up(c["q3"])
        gt = rig.zeros(3 * 48)
        steps = [
            (lambda: ctx.g1_msm_basis_dev(h, K.data_ptr(), 257, P3.data_ptr(), rig.s1.cuda_stream),
             lambda: same(rig.rows(P3, 12), c["p3"], "the sum as p[0]")),
            (lambda: ctx.pairing_many_dev(P3.data_ptr(), Q3.data_ptr(), 3, gt.data_ptr(), rig.s2.cuda_stream),
             lambda: same(rig.rows(gt, 48), c["want_many"], "the pairings"))]
        ordered(rig, "g1_msm_basis -> pairing_many", lambda: (P3.copy_(V0), gt.zero_()), steps)
        ctx.dev_status()
    finally:
        ctx.g1_basis_destroy(h)


def test_g2_msm_then_pairing_many(rig, cases, ctx):
    """The G2 sum as q[0].  Delay needed: 20 ms."""
    c = cases["g2msm_pairs"]
    ctx.g2_msm_reserve(65)
    ctx.reserve(3)
    Q, K, Q3, V0, P3 = rig.up(c["q"]), rig.up(c["k"]), rig.up(c["q3_v0"]), rig.up(c["q3_v0"]), rig.up(c["p3"])
    gt = rig.zeros(3 * 48)
    steps = [
        (lambda: ctx.g2_msm_dev(Q.data_ptr(), K.data_ptr(), 65, Q3.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(Q3, 24), c["q3"], "the sum as q[0]")),
        (lambda: ctx.pairing_many_dev(P3.data_ptr(), Q3.data_ptr(), 3, gt.data_ptr(), rig.s2.cuda_stream),
         lambda: same(rig.rows(gt, 48), c["want"], "the pairings"))]
    ordered(rig, "g2_msm -> pairing_many", lambda: (Q3.copy_(V0), gt.zero_()), steps)
    ctx.dev_status()


def test_g2_prepare_then_prepared_pairings(rig, cases, ctx):
    """A's output is the handle's table, which has no placeholder: an early B would read a
    table not yet written and miss the expected rows.  Delay needed: 20 ms (the prepare call
    allocates its table without waiting for the held stream)."""
    c = cases["prepared"]
    ctx.reserve(8)
    Qd, P, I = rig.up(c["q"]), rig.up(c["p"]), rig.up(c["idx"], np.uint32)
    gt = rig.zeros(7 * 48)
    made = []
    try:
        steps = [
            (lambda: made.append(ctx.g2_prepare_dev(Qd.data_ptr(), 3, rig.s1.cuda_stream)), None),
            (lambda: ctx.pairing_prepared_many_dev(P.data_ptr(), made[-1], I.data_ptr(), 7, gt.data_ptr(),
                                                   rig.s2.cuda_stream),
             lambda: same(rig.rows(gt, 48), c["want"], "the pairings"))]
        ordered(rig, "g2_prepare -> pairing_prepared_many", lambda: gt.zero_(), steps)
        ctx.dev_status()
    finally:
        for h in made:
            ctx.g2_prepared_destroy(h)


def test_g1_bases_prepare_then_prepared_msm(rig, cases, ctx):
    """Delay needed: 20 ms."""
    c = cases["prepared_products"]
    ctx.msm_reserve(5 * 64)
    Bd, K = rig.up(c["bases"]), rig.up(c["scal"])
    out = rig.zeros(5 * 12)
    made = []
    try:
        steps = [
            (lambda: made.append(ctx.g1_bases_prepare_dev(Bd.data_ptr(), 3, 0, rig.s1.cuda_stream)), None),
            (lambda: ctx.g1_msm_prepared_many_dev(made[-1], K.data_ptr(), 5, out.data_ptr(), 1, rig.s2.cuda_stream),
             lambda: same(rig.rows(out, 12), c["sums"], "the sums"))]
        ordered(rig, "g1_bases_prepare -> g1_msm_prepared_many", lambda: out.zero_(), steps)
    finally:
        for h in made:
            ctx.g1_prepared_destroy(h)


def test_g1_basis_prepare_then_basis_msm(rig, cases, ctx):
    """Delay needed: 20 ms."""
    c = cases["basis"]
    Bd, K = rig.up(c["bases"]), rig.up(c["k"])
    out = rig.zeros(12)
    made = []
    try:
        steps = [
            (lambda: made.append(ctx.g1_basis_prepare_dev(Bd.data_ptr(), 65, 0, rig.s1.cuda_stream)), None),
            (lambda: ctx.g1_msm_basis_dev(made[-1], K.data_ptr(), 65, out.data_ptr(), rig.s2.cuda_stream),
             lambda: same(rig.rows(out, 12), c["want"][None, :], "the sum"))]
        ordered(rig, "g1_basis_prepare -> g1_msm_basis", lambda: out.zero_(), steps)
    finally:
        for h in made:
            ctx.g1_basis_destroy(h)


@pytest.mark.parametrize("path", ["latency", "throughput"])
def test_pairing_many_then_gt_pow(rig, cases, ctx, path):
    """Seven pairings on the latency path (the default) and, with bn_set_fe_wide_max(0), through
    the throughput kernel; Gt::pow shares the pairing workspace's slots.  Delay needed: 20 ms."""
    c = cases["pow"]
    if path == "throughput":
        ctx.set_fe_wide_max(0)
    ctx.reserve(7)
    P, Q, K, ONE = rig.up(c["p7"]), rig.up(c["q7"]), rig.up(c["k7"]), rig.up(np.tile(D.gt_one(), (7, 1)))
    gt, out = rig.zeros(7 * 48), rig.zeros(7 * 48)
    steps = [
        (lambda: ctx.pairing_many_dev(P.data_ptr(), Q.data_ptr(), 7, gt.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(gt, 48), c["gt7"], "the pairings")),
        (lambda: ctx.gt_pow_many_dev(gt.data_ptr(), K.data_ptr(), 7, out.data_ptr(), rig.s2.cuda_stream),
         lambda: same(rig.rows(out, 48), c["want7"], "the powers"))]
    ordered(rig, "pairing_many (%s) -> gt_pow" % path, lambda: (gt.copy_(ONE), out.zero_()), steps)
    ctx.dev_status()


def test_pairing_products_then_gt_pow(rig, cases, ctx):
    """Delay needed: 20 ms."""
    c = cases["pow"]
    ctx.reserve(16)
    P, Q, K, ONE = rig.up(c["p11"]), rig.up(c["q11"]), rig.up(c["k5"]), rig.up(np.tile(D.gt_one(), (5, 1)))
    gt, out = rig.zeros(5 * 48), rig.zeros(5 * 48)
    steps = [
        (lambda: ctx.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), c["off5"], gt.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(gt, 48), c["prod5"], "the products")),
        (lambda: ctx.gt_pow_many_dev(gt.data_ptr(), K.data_ptr(), 5, out.data_ptr(), rig.s2.cuda_stream),
         lambda: same(rig.rows(out, 48), c["want5"], "the powers"))]
    ordered(rig, "pairing_batch_many -> gt_pow", lambda: (gt.copy_(ONE), out.zero_()), steps)
    ctx.dev_status()


def test_prepared_pairings_then_gt_pow(rig, cases, ctx):
    """Delay needed: 20 ms."""
    c, w = cases["prepared"], cases["pow"]
    ctx.reserve(8)
    h = ctx.g2_prepare(c["q"])
    try:
        P, I, K = rig.up(c["p"]), rig.up(c["idx"], np.uint32), rig.up(w["k7"])
        ONE = rig.up(np.tile(D.gt_one(), (7, 1)))
        gt, out = rig.zeros(7 * 48), rig.zeros(7 * 48)
        steps = [
            (lambda: ctx.pairing_prepared_many_dev(P.data_ptr(), h, I.data_ptr(), 7, gt.data_ptr(), rig.s1.cuda_stream),
             lambda: same(rig.rows(gt, 48), c["want"], "the pairings")),
            (lambda: ctx.gt_pow_many_dev(gt.data_ptr(), K.data_ptr(), 7, out.data_ptr(), rig.s2.cuda_stream),
             lambda: same(rig.rows(out, 48), w["want_prepared"], "the powers"))]
        ordered(rig, "pairing_prepared_many -> gt_pow", lambda: (gt.copy_(ONE), out.zero_()), steps)
        ctx.dev_status()
    finally:
        ctx.g2_prepared_destroy(h)


# ---------------------------------------------------------------- longer sequences
def test_three_streams_with_a_call_outside_the_ordering(rig, cases, ctx):
    """A (an MSM) on s1, X (bn_g1_mul_many_dev over buffers of its own, which takes no part in
    the ordering) on s2, B (a product that reads A's sum) on s3: X must not break the chain
    from A to B.  Delay needed: 20 ms."""
    c, x = cases["msm_pairs"], cases["mul"]
    ctx.set_msm_min(0)
    ctx.msm_reserve(257)
    ctx.reserve(3)
    P, K, P3, V0, Q3 = rig.up(c["p"]), rig.up(c["k"]), rig.up(c["p3_v0"]), rig.up(c["p3_v0"]), rig.up(c["q3"])
    XP, XK, xo = rig.up(x["p"]), rig.up(x["k"]), rig.zeros(33 * 12)
    gt = rig.zeros(48)
    steps = [
        (lambda: ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), 257, P3.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(P3, 12), c["p3"], "the sum as p[0]")),
        (lambda: ctx.g1_mul_many_dev(XP.data_ptr(), XK.data_ptr(), 33, xo.data_ptr(), rig.s2.cuda_stream),
         lambda: same(rig.rows(xo, 12), x["want"], "the unrelated multiplications")),
        (lambda: ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, gt.data_ptr(), None, rig.s3.cuda_stream),
         lambda: same(rig.rows(gt, 48), c["want_batch"][None, :], "the product"))]
    ordered(rig, "g1_msm | g1_mul_many | pairing_batch on three streams",
            lambda: (P3.copy_(V0), gt.zero_(), xo.zero_()), steps)


def test_three_calls_of_mixed_kinds(rig, cases, ctx):
    """A on s1, B on s2, A' on s1 again: pairings, their powers (which reuse the pairing
    workspace's slots while A' is next in line), then an MSM into another output.
    Delay needed: 20 ms."""
    c, m = cases["pow"], cases["msm_pairs"]
    ctx.set_msm_min(0)
    ctx.msm_reserve(257)
    ctx.reserve(7)
    P, Q, K, ONE = rig.up(c["p7"]), rig.up(c["q7"]), rig.up(c["k7"]), rig.up(np.tile(D.gt_one(), (7, 1)))
    MP, MK = rig.up(m["p"]), rig.up(m["k"])
    gt, out, s = rig.zeros(7 * 48), rig.zeros(7 * 48), rig.zeros(12)
    steps = [
        (lambda: ctx.pairing_many_dev(P.data_ptr(), Q.data_ptr(), 7, gt.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(gt, 48), c["gt7"], "the pairings")),
        (lambda: ctx.gt_pow_many_dev(gt.data_ptr(), K.data_ptr(), 7, out.data_ptr(), rig.s2.cuda_stream),
         lambda: same(rig.rows(out, 48), c["want7"], "the powers")),
        (lambda: ctx.g1_msm_dev(MP.data_ptr(), MK.data_ptr(), 257, s.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(s, 12), m["sum"][None, :], "the sum"))]
    ordered(rig, "pairing_many, gt_pow, g1_msm on two streams", lambda: (gt.copy_(ONE), out.zero_(), s.zero_()), steps)
    ctx.dev_status()


# ---------------------------------------------------------------- pinned-upload hand-off
# The second call waits on the host for the first call's upload of its control words (the
# header says so), so e0 is not asserted here: a call that rewrote the pinned words too early
# would make the first call compute with the second call's offsets.
@pytest.mark.parametrize("path", ["wide", "packed"])
def test_products_offsets_hand_off(rig, cases, ctx, path):
    c = cases["handoff"]
    if path == "packed":  # (0 products_min: every short product packed, however few)
        ctx.set_products_wide_max(0)
        ctx.set_products_min(0)
    ctx.reserve(32)
    P, Q = rig.up(c["p"]), rig.up(c["q"])
    ox, oy = rig.zeros(4 * 48), rig.zeros(6 * 48)
    steps = [
        (lambda: ctx.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), c["off_x"], ox.data_ptr(), rig.s1.cuda_stream),
         lambda: same(rig.rows(ox, 48), c["want_x"], "the first call's products")),
        (lambda: ctx.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), c["off_y"], oy.data_ptr(), rig.s2.cuda_stream),
         lambda: same(rig.rows(oy, 48), c["want_y"], "the second call's products"))]
    ctx.products_routes()
    ordered(rig, "products hand-off (%s)" % path, lambda: (ox.zero_(), oy.zero_()), steps, assert_e0=False)
    wide, packed, alone = ctx.products_routes()
    assert alone == 0 and (packed == 0 if path == "wide" else wide == 0) and wide + packed > 0
    ctx.dev_status()


@pytest.mark.parametrize("path", ["wide", "packed"])
def test_prepared_products_map_hand_off(rig, cases, ctx, path):
    c = cases["handoff"]
    if path == "packed":
        ctx.set_products_wide_max(0)
    ctx.reserve(32)
    h = ctx.g2_prepare(c["table"])
    try:
        P, FX, FY = rig.up(c["p"]), rig.up(c["fresh_x"]), rig.up(c["fresh_y"])
        ox, oy = rig.zeros(4 * 48), rig.zeros(6 * 48)
        steps = [
            (lambda: ctx.pairing_batch_prepared_many_dev(P.data_ptr(), FX.data_ptr(), h, c["qidx_x"], c["off_x"],
                                                         ox.data_ptr(), rig.s1.cuda_stream),
             lambda: same(rig.rows(ox, 48), c["want_px"], "the first call's products")),
            (lambda: ctx.pairing_batch_prepared_many_dev(P.data_ptr(), FY.data_ptr(), h, c["qidx_y"], c["off_y"],
                                                         oy.data_ptr(), rig.s2.cuda_stream),
             lambda: same(rig.rows(oy, 48), c["want_py"], "the second call's products"))]
        ordered(rig, "prepared products hand-off (%s)" % path, lambda: (ox.zero_(), oy.zero_()), steps, assert_e0=False)
        ctx.dev_status()
    finally:
        ctx.g2_prepared_destroy(h)


def test_msm_many_words_hand_off(rig, cases, ctx):
    c = cases["handoff"]
    ctx.g1_msm_many_reserve(15, 5)
    P, K = rig.up(c["mp"]), rig.up(c["mk"])
    ox, oy = rig.zeros(3 * 12), rig.zeros(5 * 12)
    steps = [
        (lambda: ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), c["moff_x"], ox.data_ptr(), 1, rig.s1.cuda_stream),
         lambda: same(rig.rows(ox, 12), c["want_mx"], "the first call's sums")),
        (lambda: ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), c["moff_y"], oy.data_ptr(), 1, rig.s2.cuda_stream),
         lambda: same(rig.rows(oy, 12), c["want_my"], "the second call's sums"))]
    ordered(rig, "msm_many hand-off", lambda: (ox.zero_(), oy.zero_()), steps, assert_e0=False)


# ---------------------------------------------------------------- calls documented to wait
def _queued_pairings(rig, cases, ctx):
    """Seven pairings warmed up, then queued on s1 behind the delay; e1 follows them on s1."""
    c = cases["pow"]
    P, Q, gt = rig.up(c["p7"]), rig.up(c["q7"]), rig.zeros(7 * 48)
    call = lambda: ctx.pairing_many_dev(P.data_ptr(), Q.data_ptr(), 7, gt.data_ptr(), rig.s1.cuda_stream)  # noqa: E731
    check = lambda: same(rig.rows(gt, 48), c["gt7"], "the queued pairings")  # noqa: E731
    warm(rig, gt.zero_, [(call, check)])
    gt.zero_()
    rig.sync()
    rig.hold(DELAYS_MS[0])
    call()
    return rig.event(rig.s1), check, (P, Q, gt)


def test_dev_status_on_another_stream_waits(rig, cases, ctx):
    e1, check, _keep = _queued_pairings(rig, cases, ctx)
    ctx.dev_status(rig.s2.cuda_stream)
    assert e1.query()
    check()


def test_regrowing_the_pairing_workspace_waits(rig, cases, ctx):
    """1,025 pairs on s2 against a workspace of 1,024 while seven pairings are queued on s1."""
    c = cases["pow"]
    n = cases["regrow"]["n_pairs"]
    reps = n // 7 + 1
    P2, Q2 = rig.up(np.tile(c["p7"], (reps, 1))[:n]), rig.up(np.tile(c["q7"], (reps, 1))[:n])
    big = rig.zeros(n * 48)
    e1, check, _keep = _queued_pairings(rig, cases, ctx)
    ctx.pairing_many_dev(P2.data_ptr(), Q2.data_ptr(), n, big.data_ptr(), rig.s2.cuda_stream)
    assert e1.query()
    check()
    ctx.dev_status()
    same(rig.rows(big, 48), np.tile(c["gt7"], (reps, 1))[:n], "the larger batch")


def test_regrowing_the_msm_workspace_waits(rig, cases, ctx):
    """Six terms on s2 against an MSM workspace sized for five while the pairings are queued."""
    m, r = cases["msm_pairs"], cases["regrow"]
    P, K, s = rig.up(m["p"][:6]), rig.up(m["k"][:6]), rig.zeros(12)
    ctx.msm_reserve(5)
    ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), 5, s.data_ptr(), rig.s2.cuda_stream)
    rig.sync()
    same(rig.rows(s, 12), r["msm5"][None, :], "five terms")
    e1, check, _keep = _queued_pairings(rig, cases, ctx)
    ctx.g1_msm_dev(P.data_ptr(), K.data_ptr(), 6, s.data_ptr(), rig.s2.cuda_stream)
    assert e1.query()
    check()
    rig.sync()
    same(rig.rows(s, 12), r["msm6"][None, :], "six terms")


def test_g2_prepared_destroy_waits(rig, cases, ctx):
    c = cases["prepared"]
    h = ctx.g2_prepare(c["q"])
    P, I, gt = rig.up(c["p"]), rig.up(c["idx"], np.uint32), rig.zeros(7 * 48)
    call = lambda: ctx.pairing_prepared_many_dev(P.data_ptr(), h, I.data_ptr(), 7, gt.data_ptr(), rig.s1.cuda_stream)  # noqa: E731
    call()
    rig.sync()
    gt.zero_()
    rig.sync()
    rig.hold(DELAYS_MS[0])
    call()
    e1 = rig.event(rig.s1)
    ctx.g2_prepared_destroy(h)
    assert e1.query()
    same(rig.rows(gt, 48), c["want"], "the pairings that read the handle")


def test_g1_prepared_destroy_waits(rig, cases, ctx):
    c = cases["prepared_products"]
    h = ctx.g1_bases_prepare(c["bases"])
    K, out = rig.up(c["scal"]), rig.zeros(5 * 12)
    call = lambda: ctx.g1_msm_prepared_many_dev(h, K.data_ptr(), 5, out.data_ptr(), 1, rig.s1.cuda_stream)  # noqa: E731
    call()
    rig.sync()
    out.zero_()
    rig.sync()
    rig.hold(DELAYS_MS[0])
    call()
    e1 = rig.event(rig.s1)
    ctx.g1_prepared_destroy(h)
    assert e1.query()
    same(rig.rows(out, 12), c["sums"], "the sums that read the handle")


def test_g1_basis_destroy_waits(rig, cases, ctx):
    c = cases["basis"]
    h = ctx.g1_basis_prepare(c["bases"])
    K, out = rig.up(c["k"]), rig.zeros(12)
    call = lambda: ctx.g1_msm_basis_dev(h, K.data_ptr(), 65, out.data_ptr(), rig.s1.cuda_stream)  # noqa: E731
    call()
    rig.sync()
    out.zero_()
    rig.sync()
    rig.hold(DELAYS_MS[0])
    call()
    e1 = rig.event(rig.s1)
    ctx.g1_basis_destroy(h)
    assert e1.query()
    same(rig.rows(out, 12), c["want"][None, :], "the sum that reads the handle")


# ---------------------------------------------------------------- the sticky outcome
@pytest.mark.parametrize("middle", ["pairing_batch", "miller_loop_batch"])
def test_sticky_outcome_survives_a_call_with_its_own_status_word(rig, cases, ctx, middle):
    """bn_pairing_prepared_many_dev with one index past the handle's count (clamped, that row
    zero), then bn_pairing_batch_dev / bn_miller_loop_batch_dev on good pairs with a status word,
    then bn_dev_status: the status word reports the middle call alone, BN_OK, and bn_dev_status
    still reports the bad index, once.  Before the fix the middle call cleared the shared outcome
    word and the first bn_dev_status returned BN_OK (0) instead of BN_ERR_INVALID_ARGUMENT (1)."""
    c, m = cases["prepared"], cases["msm_pairs"]
    h = ctx.g2_prepare(c["q"])
    try:
        P, I, gt = rig.up(c["p"]), rig.up(c["bad_idx"], np.uint32), rig.zeros(7 * 48)
        P3, Q3, out = rig.up(m["p3"]), rig.up(m["q3"]), rig.zeros(48)
        st = rig.torch.full((1,), -1, dtype=rig.torch.int32, device=rig.dev)
        ctx.pairing_prepared_many_dev(P.data_ptr(), h, I.data_ptr(), 7, gt.data_ptr())
        if middle == "pairing_batch":
            ctx.pairing_batch_dev(P3.data_ptr(), Q3.data_ptr(), 3, out.data_ptr(), st.data_ptr())
            want = m["want_batch"]
        else:
            ctx.miller_loop_batch_dev(Q3.data_ptr(), P3.data_ptr(), 3, out.data_ptr(), st.data_ptr())
            want = m["want_miller"]
        first = ctx._L.bn_dev_status(ctx.handle, None)
        second = ctx._L.bn_dev_status(ctx.handle, None)
        rig.sync()
        print("sticky outcome after %s_dev: first bn_dev_status %d, second %d, status word %d"
              % (middle, first, second, int(st.item())))
        assert int(st.item()) == OK
        same(rig.rows(out, 48), want[None, :], "the middle call's result")
        same(rig.rows(gt, 48), c["bad_want"], "the prepared pairings, the bad row zero")
        assert first == INVALID
        assert second == OK
    finally:
        ctx.g2_prepared_destroy(h)
