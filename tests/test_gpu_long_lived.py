"""One context kept alive through everything a verifier service does to it.

test_one_context_runs_the_script: the script of tests/long_lived_cases.py -- every kind of call
at sizes that go up and down, settings changed and put back, handles made and destroyed, failures
in between -- on ONE Context, forward, then with the middle reversed, then (the calls bn254mi.h
lists as ordered across streams) through their _dev forms on two alternating torch streams
with no host synchronization between the steps.  Every step is compared with the oracle's stored
answer; a failure names the step, its size and the step before it.

The three epoch tests create their contexts under $BN254MI_TAIL_EPOCH_WRAP=3, so that the counter
that stamps the words k_fe_ds and k_seg_tail poll (bn_ctx.tail_epoch, csrc/tail_epoch.h) returns
to 1 on every third tail launch.  The kernels do not rewrite every word on every launch, so a word
stamped at epoch 1 by a large launch survives smaller launches at epochs 2 and 3 and would be
taken as published by the next launch at epoch 1 -- a wrong Gt, or a hand-off wait that runs out
(BN_ERR_INTERNAL) -- unless both buffers are cleared on the wrap.  Each test puts a large launch
at epoch 1, small ones at 2 and 3, and a large one on other inputs at 1 again, against the
oracle."""
import ctypes

import numpy as np
import pytest

from tests import long_lived_cases as L

pytestmark = pytest.mark.gpu
OK, INVALID, TO_AFFINE = L.OK, L.INVALID, L.TO_AFFINE
SETTERS = {"fe_wide_max": "set_fe_wide_max", "msm_min": "set_msm_min", "msm_run_max": "set_msm_run_max",
           "msm_window": "set_msm_window", "msm_many_max": "set_msm_many_max", "products_wide_max": "set_products_wide_max",
           "products_min": "set_products_min", "fq12_op_unit": "set_fq12_op_unit"}
PREPARE = {"g2_prepare": ("g2_prepare", "q"), "g1_bases_prepare": ("g1_bases_prepare", "bases"),
           "g1_basis_prepare": ("g1_basis_prepare", "bases")}
DESTROY = {"g2_prepared_destroy": "g2_prepared_destroy", "g1_prepared_destroy": "g1_prepared_destroy",
           "g1_basis_destroy": "g1_basis_destroy"}


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.ndim == 1:
        got, want = got[None, :], want[None, :]
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, "%s: rows %s of %d differ from the oracle" % (what, bad[:8].tolist(), got.shape[0])


class Dev:
    """Upload and read-back helpers over torch tensors of 64-bit words."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)

    def up(self, a, dtype=np.uint64):
        a = np.ascontiguousarray(a, dtype=dtype)
        view = {np.uint64: np.int64, np.uint32: np.int32}[dtype]
        return self.torch.from_numpy(a.view(view).reshape(-1).copy()).to(self.dev)

    def zeros(self, words):
        return self.torch.zeros(words, dtype=self.torch.int64, device=self.dev)

    def status(self):
        return self.torch.full((1,), -1, dtype=self.torch.int32, device=self.dev)

    def sync(self):
        self.torch.cuda.synchronize(self.dev)

    @staticmethod
    def rows(t, width):
        return t.cpu().numpy().view(np.uint64).reshape(-1, width)


@pytest.fixture(scope="module")
def dev():
    return Dev()


@pytest.fixture(scope="module")
def passes():
    return L.order(False), L.order(True)


# ---------------------------------------------------------------- the host forms
def run_churn(ctx, s, what):
    """Seven handles, at most three alive at once; a destroyed handle's table memory is free for
    the next prepare call while the other handles are in use."""
    g2, g1p, basis = s["g2"], s["g1p"], s["basis"]
    idx = np.arange(2, dtype=np.uint32)
    use_g2 = lambda h, d: same(ctx.pairing_prepared_many(d["p"], h, idx), d["want"], what + ": a prepared G2 handle")  # noqa: E731
    use_g1 = lambda h, d: same(ctx.g1_msm_prepared_many(h, d["scal"]), d["want"], what + ": a prepared G1 handle")  # noqa: E731
    use_b = lambda h, d: same(ctx.g1_msm_basis(h, d["k"]), d["want"], what + ": a basis handle")  # noqa: E731
    a, b, c = ctx.g2_prepare(g2[0]["q"]), ctx.g1_bases_prepare(g1p[0]["bases"]), ctx.g1_basis_prepare(basis[0]["bases"])
    use_g2(a, g2[0]), use_g1(b, g1p[0]), use_b(c, basis[0])
    ctx.g2_prepared_destroy(a)
    a2 = ctx.g2_prepare(g2[1]["q"])
    use_g1(b, g1p[0]), use_g2(a2, g2[1])
    ctx.g1_prepared_destroy(b)
    b2 = ctx.g1_bases_prepare(g1p[1]["bases"])
    ctx.g1_basis_destroy(c)
    c2 = ctx.g1_basis_prepare(basis[1]["bases"])
    use_g2(a2, g2[1]), use_g1(b2, g1p[1]), use_b(c2, basis[1])
    ctx.g2_prepared_destroy(a2)
    a3 = ctx.g2_prepare(g2[2]["q"])
    use_g2(a3, g2[2]), use_b(c2, basis[1]), use_g1(b2, g1p[1])
    ctx.g2_prepared_destroy(a3)
    ctx.g1_prepared_destroy(b2)
    ctx.g1_basis_destroy(c2)


def check_routes(ctx, s, what):
    got = ctx.products_routes()
    assert got == tuple(s["routes"]), "%s: routes (wide, packed, alone) %s, expected %s" % (what, got, s["routes"])


def run_host(ctx, dev, H, dead, s, what):
    """One step through the host-buffer form of its call, checked against s["want"]."""
    from substrate_bn import BnError
    kind, lib = s["kind"], ctx._L
    if kind.startswith("set:"):
        getattr(ctx, SETTERS[s["name"]])(s["value"])
    elif kind in PREPARE:
        method, key = PREPARE[kind]
        H[s["name"]] = getattr(ctx, method)(s[key])
    elif kind in DESTROY:
        dead[s["name"]] = H.pop(s["name"])
        getattr(ctx, DESTROY[kind])(dead[s["name"]])
    elif kind == "handle_churn":
        run_churn(ctx, s, what)
    elif kind == "pairing_many":
        same(ctx.pairing_many(s["p"], s["q"]), s["want"], what)
    elif kind == "pairing_batch":
        same(ctx.pairing_batch(s["p"], s["q"]), s["want"], what)
    elif kind == "miller_loop_batch":
        same(ctx.miller_loop_batch(s["q"], s["p"]), s["want"], what)
    elif kind == "miller_loop_many":
        same(ctx.miller_loop_many(s["p"], s["q"]), s["want"], what)
    elif kind == "final_exponentiation_many":
        out, ok = ctx.final_exponentiation_many(s["f"])
        same(ok, s["want"][1], what + " (ok)")
        same(out, s["want"][0], what)
    elif kind == "g2_precompute_many":
        same(ctx.g2_precompute_many(s["q"]), s["want"], what)
    elif kind == "pairing_prepared_many":
        same(ctx.pairing_prepared_many(s["p"], H[s["handle"]], s["idx"]), s["want"], what)
    elif kind == "miller_loop_prepared_many":
        same(ctx.miller_loop_prepared_many(s["p"], H[s["handle"]], s["idx"]), s["want"], what)
    elif kind == "pairing_batch_many":
        ctx.products_routes()
        same(ctx.pairing_batch_many(s["p"], s["q"], s["off"]), s["want"], what)
        check_routes(ctx, s, what)
    elif kind == "pairing_batch_prepared_many":
        ctx.products_routes()
        same(ctx.pairing_batch_prepared_many(s["p"], s["q"], H[s["handle"]], s["qidx"], s["off"]), s["want"], what)
        check_routes(ctx, s, what)
    elif kind in ("g1_mul_many", "g2_mul_many", "g1_msm", "g2_msm"):
        same(getattr(ctx, kind)(s["p"], s["k"]), s["want"], what)
    elif kind == "g1_msm_prepared_many":
        same(ctx.g1_msm_prepared_many(H[s["handle"]], s["scal"]), s["want"], what)
    elif kind == "g1_msm_many":
        same(ctx.g1_msm_many(s["p"], s["k"], s["off"]), s["want"], what)
    elif kind == "g1_msm_basis":
        same(ctx.g1_msm_basis(H[s["handle"]], s["k"]), s["want"], what)
    elif kind in ("g1_group", "g2_group"):
        for op, want in zip(L.GROUP_OPS, s["want"]):
            same(ctx.group_op_many(kind[:2], op, s["a"], s["b"]), want, "%s (%s)" % (what, op))
    elif kind == "fq12_op_many":
        for op in L.FQ12_OPS:
            same(ctx.fq12_op_many(op, s["a"], s["b"] if op == "mul" else None), s["want"][op], "%s (%s)" % (what, op))
    elif kind == "gt_pow_many":
        same(ctx.gt_pow_many(s["a"], s["k"]), s["want"], what)
    elif kind in ("fq_sqrt_many", "fq2_sqrt_many"):
        out, ok = getattr(ctx, kind)(s["a"])
        ref, rok = s["want"]
        same(ok.astype(bool), rok, what + " (ok)")
        same(out[rok], ref[rok], what)
    elif kind in ("g1_from_compressed_many", "g2_from_compressed_many"):
        out, st = getattr(ctx, kind)(s["b"])
        same(st, s["want"][1], what + " (status)")
        same(out, s["want"][0], what)
    # ---- the outcome steps
    elif kind == "err:miller_loop_batch_zero":
        with pytest.raises(BnError) as e:
            ctx.miller_loop_batch(s["q"], s["p"])
        assert e.value.code == s["code"], what
    elif kind == "err:products_offsets":
        p, q, off = (np.ascontiguousarray(s[k]) for k in ("p", "q", "off"))
        out = np.zeros((off.shape[0] - 1, 48), np.uint64)
        assert lib.bn_pairing_batch_many(ctx.handle, ptr(p), ptr(q), ptr(off), off.shape[0] - 1, ptr(out)) == s["code"], what
        assert not out.any(), what
    elif kind == "err:prepared_index_host":
        p, idx = np.ascontiguousarray(s["p"]), np.ascontiguousarray(s["idx"])
        out = np.zeros((p.shape[0], 48), np.uint64)
        rc = lib.bn_pairing_prepared_many(ctx.handle, ptr(p), H[s["handle"]], ptr(idx), p.shape[0], ptr(out))
        assert rc == s["code"], what
    elif kind == "err:prepared_index_dev":
        P, I, out = dev.up(s["p"]), dev.up(s["idx"], np.uint32), dev.zeros(s["size"] * 48)
        dev.sync()
        ctx.pairing_prepared_many_dev(P.data_ptr(), H[s["handle"]], I.data_ptr(), s["size"], out.data_ptr())
        first, second = lib.bn_dev_status(ctx.handle, None), lib.bn_dev_status(ctx.handle, None)
        assert (first, second) == (s["code"], OK), "%s: bn_dev_status gave %d then %d" % (what, first, second)
        same(dev.rows(out, 48), s["want"], what)
    elif kind == "err:destroyed_handle":
        k = np.ascontiguousarray(s["k"])
        out = np.zeros(12, np.uint64)
        assert lib.bn_g1_msm_basis(ctx.handle, dead[s["handle"]], ptr(k), k.shape[0], ptr(out)) == INVALID, what
        assert not out.any(), what
    else:
        raise AssertionError("no runner for " + kind)


def run_pass(ctx, dev, steps, name):
    H, dead, prev = {}, {}, None
    for i, s in enumerate(steps):
        what = "%s pass, step %d (%s) after %s" % (name, i, L.step_label(s), L.step_label(prev))
        try:
            run_host(ctx, dev, H, dead, s, what)
        except AssertionError:
            raise
        except Exception as e:  # a call that failed where the oracle has an answer
            raise AssertionError("%s: %s: %s" % (what, type(e).__name__, e))
        prev = s
    assert not H, "handles left alive: %s" % sorted(H)


# ---------------------------------------------------------------- the device forms
def run_dev_pass(ctx, dev, steps):
    """The ordered calls of `steps` through their _dev forms, alternating between two streams, no
    host synchronization by the test between them (bn_dev_status, where the script reads it, and
    the destroy calls wait by themselves); every step writes its own output buffer, all compared
    after one synchronization at the end.  Inputs go up beforehand."""
    torch = dev.torch
    streams = [torch.cuda.Stream(dev.dev), torch.cuda.Stream(dev.dev)]
    todo = [s for s in steps if s["kind"] in L.DEV_KINDS or s["kind"].startswith("set:") or s["kind"] in DESTROY]
    bufs = []
    for s in todo:
        b = {}
        for key, dt in (("p", np.uint64), ("q", np.uint64), ("k", np.uint64), ("a", np.uint64), ("bases", np.uint64),
                        ("scal", np.uint64), ("idx", np.uint32)):
            if key in s and s[key] is not None and s["kind"] in L.DEV_KINDS:
                b[key] = dev.up(s[key], dt)
        if "want" in s:
            b["out"] = dev.zeros(int(np.asarray(s["want"]).size))
        if s["kind"] in ("pairing_batch", "miller_loop_batch"):
            b["st"] = dev.status()
        bufs.append(b)
    dev.sync()
    H, checks, prev, n = {}, [], None, 0
    ctx.products_routes()
    for i, (s, b) in enumerate(zip(todo, bufs)):
        kind = s["kind"]
        what = "device pass, step %d (%s) after %s" % (i, L.step_label(s), L.step_label(prev))
        st = streams[n % 2].cuda_stream
        dp = lambda key: b[key].data_ptr() if key in b and b[key].numel() else None  # noqa: E731
        try:
            if kind.startswith("set:"):
                getattr(ctx, SETTERS[s["name"]])(s["value"])
                continue
            if kind in DESTROY:
                getattr(ctx, DESTROY[kind])(H.pop(s["name"]))
                continue
            n += 1
            if kind == "g2_prepare":
                H[s["name"]] = ctx.g2_prepare_dev(dp("q"), s["size"], st)
            elif kind == "g1_bases_prepare":
                H[s["name"]] = ctx.g1_bases_prepare_dev(dp("bases"), s["size"], 0, st)
            elif kind == "g1_basis_prepare":
                H[s["name"]] = ctx.g1_basis_prepare_dev(dp("bases"), s["size"], 0, st)
            elif kind == "pairing_many":
                ctx.pairing_many_dev(dp("p"), dp("q"), s["size"], dp("out"), st)
            elif kind == "pairing_batch":
                ctx.pairing_batch_dev(dp("p"), dp("q"), s["size"], dp("out"), b["st"].data_ptr(), st)
            elif kind == "miller_loop_batch":
                ctx.miller_loop_batch_dev(dp("q"), dp("p"), s["size"], dp("out"), b["st"].data_ptr(), st)
            elif kind == "pairing_batch_many":
                ctx.pairing_batch_many_dev(dp("p"), dp("q"), s["off"], dp("out"), st)
                check_routes(ctx, s, what)
            elif kind == "pairing_batch_prepared_many":
                ctx.pairing_batch_prepared_many_dev(dp("p"), dp("q"), H[s["handle"]], s["qidx"], s["off"], dp("out"), st)
                check_routes(ctx, s, what)
            elif kind == "pairing_prepared_many":
                ctx.pairing_prepared_many_dev(dp("p"), H[s["handle"]], dp("idx"), s["size"], dp("out"), st)
            elif kind == "err:prepared_index_dev":
                ctx.pairing_prepared_many_dev(dp("p"), H[s["handle"]], dp("idx"), s["size"], dp("out"), st)
                first, second = ctx._L.bn_dev_status(ctx.handle, None), ctx._L.bn_dev_status(ctx.handle, None)
                assert (first, second) == (s["code"], OK), "%s: bn_dev_status gave %d then %d" % (what, first, second)
            elif kind in ("g1_msm", "g2_msm"):
                getattr(ctx, kind + "_dev")(dp("p"), dp("k"), s["size"], dp("out"), st)
            elif kind == "g1_msm_prepared_many":
                ctx.g1_msm_prepared_many_dev(H[s["handle"]], dp("scal"), s["size"], dp("out"), 1, st)
            elif kind == "g1_msm_many":
                ctx.g1_msm_many_dev(dp("p"), dp("k"), s["off"], dp("out"), 1, st)
            elif kind == "g1_msm_basis":
                ctx.g1_msm_basis_dev(H[s["handle"]], dp("k"), s["size"], dp("out"), st)
            elif kind == "gt_pow_many":
                ctx.gt_pow_many_dev(dp("a"), dp("k"), s["size"], dp("out"), st)
            else:
                raise AssertionError("no device runner for " + kind)
        except AssertionError:
            raise
        except Exception as e:
            raise AssertionError("%s: %s: %s" % (what, type(e).__name__, e))
        if "want" in s:
            checks.append((what, s, b))
        prev = s
    assert not H, "handles left alive: %s" % sorted(H)
    dev.sync()
    ctx.dev_status()
    for what, s, b in checks:
        want = np.asarray(s["want"])
        same(dev.rows(b["out"], want.shape[-1]).reshape(want.shape), want, what)
        if "st" in b:
            assert int(b["st"].item()) == OK, what + " (status word)"
    return len(checks)


def test_one_context_runs_the_script(dev, passes):
    """Forward, reverse and device-form passes on one Context, which is never recreated."""
    from substrate_bn import Context
    fwd, rev = passes
    ctx = Context(0)
    try:
        run_pass(ctx, dev, fwd, "forward")
        run_pass(ctx, dev, rev, "reverse")
        n = run_dev_pass(ctx, dev, fwd)
        print("%d steps forward, %d in reverse, %d device-form results compared" % (len(fwd), len(rev), n))
        assert n >= 60
        # and the context is still good for the host forms
        run_pass(ctx, dev, fwd[:4] + fwd[-6:], "closing")
    finally:
        ctx.close()


# ---------------------------------------------------------------- the epoch wrap
def wrap_context(monkeypatch, wrap):
    from substrate_bn import Context
    if wrap is None:
        monkeypatch.delenv("BN254MI_TAIL_EPOCH_WRAP", raising=False)
    else:
        monkeypatch.setenv("BN254MI_TAIL_EPOCH_WRAP", str(wrap))
    return Context(0)


def fe_ds_sizes(dev):
    """(a, b): a pairs take three blocks each (3 a kLatPairs <= lat_w1_max, i.e. 3 a <= CUs), b
    pairs one block each."""
    cus = dev.torch.cuda.get_device_properties(0).multi_processor_count
    a, b = min(64, cus // 3), min(256, cus // 3 + 1)
    assert 1 <= a and 2 * a <= 128 and 3 * a <= cus < 3 * b and b <= 256, (cus, a, b)
    return a, b


def fe_ds_calls(ctx, a, b):
    """The tail launches of the k_fe_ds test, in order, as (label, call); every call is one
    launch of k_fe_ds.  Under a wrap of 3 the epochs are 1, 2, 3, 1, ...: the calls marked (1)
    run at epoch 1, the launch that follows a clear from the second one on."""
    pl = L.pool()
    P, Q, E, ML = pl.P, pl.Q, pl.E, pl.ML

    def pm(at, n):
        return ("pairing_many of %d pairs from row %d" % (n, at),
                lambda: same(ctx.pairing_many(P[at:at + n], Q[at:at + n]), E[at:at + n], "pairing_many"))

    def fe(at, n):
        f, want, ok = ML[at:at + n].copy(), E[at:at + n].copy(), np.ones(n, np.uint8)
        for z in (1, n - 2):
            f[z], want[z], ok[z] = 0, 0, 0

        def call():
            out, got_ok = ctx.final_exponentiation_many(f)
            same(got_ok, ok, "final_exponentiation_many (ok)")
            same(out, want, "final_exponentiation_many")
        return ("final_exponentiation_many of %d rows from row %d, two of them zero" % (n, at), call)
    return [pm(0, a),            # (1) three blocks per pair: every pair's role word and channel stamped 1
            pm(200, 1), pm(201, 1),
            pm(a, a),            # (1) other pairs over the words the first call stamped
            pm(257 - b, b),      # one block per pair: role words only
            pm(202, 1),
            pm(0, a),            # (1)
            pm(203, 1),
            fe(a, a),            # run_fe's launch site
            fe(0, a),            # (1)
            pm(204, 1), pm(205, 1),
            pm(a, a)]            # (1)


def test_epoch_wrap_k_fe_ds(dev, monkeypatch):
    a, b = fe_ds_sizes(dev)
    ctx = wrap_context(monkeypatch, 3)
    try:
        calls = fe_ds_calls(ctx, a, b)
        assert len(calls) >= 9
        for i, (label, call) in enumerate(calls):
            try:
                call()
            except Exception as e:
                raise AssertionError("tail launch %d (epoch %d): %s: %s" % (i, i % 3 + 1, label, e))
        print("a = %d, b = %d: %d tail launches, %d wraps" % (a, b, len(calls), (len(calls) - 1) // 3))
    finally:
        ctx.close()


def seg_tail_calls(ctx):
    """The tail launches of the k_seg_tail test.  pairing_batch under bn_set_latency_max(24): 25, 40
    and 64 terms run the segmented product, whose plan has S = 16 segments (k_seg_tail writes
    the links and node words of 16 segments); 1, 3 and 24 terms run the latency product, whose
    tail has S = 1 (no link written).  pairing_many of 7 pairs launches k_fe_ds on the same
    counter."""
    pl, prod = L.pool(), L.seg_tail_products()
    P, Q, E = pl.P, pl.Q, pl.E
    assert set(n for _, n in prod) == set(L.SEG_TERMS["S=1"]) | set(L.SEG_TERMS["S=16"])

    def pb(at, n):
        S = 1 if n <= L.SEG_LATENCY_MAX else 16
        return ("pairing_batch of %d terms from row %d (S = %d)" % (n, at, S),
                lambda: same(ctx.pairing_batch(P[at:at + n], Q[at:at + n]), prod[(at, n)], "pairing_batch"))

    def pm(at, n):
        return ("pairing_many of %d pairs from row %d (k_fe_ds)" % (n, at),
                lambda: same(ctx.pairing_many(P[at:at + n], Q[at:at + n]), E[at:at + n], "pairing_many"))
    return [pb(0, 40),       # (1) S = 16
            pb(40, 24), pb(64, 3),      # S = 1, twice
            pb(100, 40),     # (1) S = 16 on other terms
            pb(140, 25), pb(67, 1),
            pb(165, 64),     # (1) S = 16
            pm(210, 7), pb(70, 24),     # the two kernels alternately on one counter
            pm(220, 7),      # (1) k_fe_ds on the launch that follows the clear
            pb(94, 3), pm(230, 1),
            pb(230, 25)]     # (1) S = 16


def test_epoch_wrap_k_seg_tail(monkeypatch):
    ctx = wrap_context(monkeypatch, 3)
    try:
        ctx.set_latency_max(L.SEG_LATENCY_MAX)
        calls = seg_tail_calls(ctx)
        for i, (label, call) in enumerate(calls):
            try:
                call()
            except Exception as e:
                raise AssertionError("tail launch %d (epoch %d): %s: %s" % (i, i % 3 + 1, label, e))
        assert (len(calls) - 1) // 3 >= 3
    finally:
        ctx.close()


def test_default_wrap_is_unchanged(dev, monkeypatch):
    """With the switch unset the same calls give the same results (the counter runs 1, 2, ...
    as before and nothing is cleared within any test's reach)."""
    a, b = fe_ds_sizes(dev)
    ctx = wrap_context(monkeypatch, None)
    try:
        for label, call in fe_ds_calls(ctx, a, b)[:6]:
            call()
        ctx.set_latency_max(L.SEG_LATENCY_MAX)
        for label, call in seg_tail_calls(ctx)[:6]:
            call()
    finally:
        ctx.close()
