#!/usr/bin/env python3
"""Device time of bn_g1_msm_dev (or, with --group g2, bn_g2_msm_dev) per size
(HBM-resident inputs, torch events on the launch stream, the group's reserve call and a
warm-up before timing), alternating in one process:
  small    the small path forced (bn_g1_mul_many's kernels, an addition tree of
           k_g1_op, normalize): what a caller composes from bn_g1_mul_many_dev,
           ceil(log2 n) x bn_g1_add_many_dev and bn_g1_normalize_many_dev
           (g2: the same from the bn_g2_* calls)
  c=K      the bucket path forced at window width K
  default  a context with untouched settings (the window table and the threshold)
Before a size is timed every form must return the same 96 (g2: 192) bytes, else the
script exits non-zero.  One JSON line per size, then one line for all-equal scalars at
--skew terms (every window has one bucket that holds every term; --run-cap measures the
skew patterns in full).  `frac` is the integer-VALU roofline fraction as DESIGN.md §4.5 counts it:
algorithmic Fq products x 128 MAD32 over the time, against 39.3 T MAD32/s.

With --run-cap the sweep is over the run cap instead (bn_set_msm_run_max; msm.h), on the
bucket path at the automatic window, alternating in one process:
  unsplit  BN_MSM_RUN_UNSPLIT: one lane per key whatever its run
  default  the default rule max(128, 2 * ceil(n / 2^(c-1)))
  L0=K     the same rule with K for the 128, set as an explicit cap
one JSON line per size with `default_in_unsplit_spread` (the default's median inside the
unsplit form's own min .. max), then at --skew terms four skewed scalar patterns (all equal,
all 1, half 1 / half uniform, 1 % equal to r - 1), each as unsplit (one repetition: it takes
seconds), split (the default cap) and small (the small path), after checking that the three
return the same bytes.

With --basis the comparison is bn_g1_msm_dev (a context with untouched settings: its automatic
width) against bn_g1_msm_basis_dev over a bn_g1_basis of the same n bases, or with
--group g2 bn_g2_msm_dev against bn_g2_msm_basis_dev over a bn_g2_basis, by
the same protocol: HBM-resident inputs, workspace reserved, a warm-up of every form, --reps
repetitions per form alternating in one process, torch events on the launch stream, median
ms, and a check first that every form returns the same bytes.  The basis form runs at its
default width and at the two widths on either side (--basis-windows lists other widths).  One
JSON line per size with the prepare time (events around the _dev prepare call, its table
allocation included) and table bytes of every width, then at --skew terms
the four skewed patterns of --run-cap.  `gain_outside_spread`: the default-width basis form's
median is below bn_g1_msm's by more than the wider of the two forms' own min .. max spreads.

With --basis-many the comparison is bn_g1_msm_basis_many_dev against a loop of m
bn_g1_msm_basis_dev calls on the same handle (n bases at its default width) and the same m x n
scalars, by the same protocol: HBM-resident inputs, the workspace reserved, a warm-up of both
forms that is also the byte-equality check of all m outputs, --reps repetitions alternating
the two forms in one process, events on the launch stream, median ms.  One JSON line per
(m, n) of --many-m x --sizes (default 2,8,32,128 x 2^10,2^12,2^14,2^16,2^18) and per shape of
--many-shapes (default 9x65536, the PLONK shape); a shape whose scalars, table or workspace
do not fit is skipped with a line that says so.  `gain_outside_spread`: the batched form's
median is below the loop's by more than the wider of the two forms' own min .. max spreads.
--many-set-keys lists bounds on S * nkeys (the launch set's bucket memory) to sweep at every
shape instead, each forced through bn_set_msm_basis_many_set.  --many-loop-only times the loop
alone (a library that predates the batched call, through BN254MI_LIB; or a profiler run of
that form alone), --many-only the batched form alone, without the check.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "paritytech-bn_amd"))
sys.path.insert(0, ROOT)

PEAK_MAD32 = 39.3e12
# Fq products of jac_add / jac_double (curve.h): 11 products + 5 squares, 2 products + 5 squares.
# g2: an Fq2 product is two Fq products on each lane of the pair (fq2_split.h) = 4, an Fq2
# square one on each lane (fq2.rs:105-117) = 2
OPS = {"g1": (16, 7), "g2": (11 * 4 + 5 * 2, 2 * 4 + 5 * 2)}
SEGMENT = 16      # kMsmSegment (msm.h)
# capi_msm.hip MsmGroup<P>::auto_window: (first n of the next row, c)
AUTO_WINDOW = {"g1": ((6144, 10), (92682, 12), (370728, 14), (741455, 15)),
               "g2": ((1449, 10), (23171, 11), (46341, 12), (370728, 14), (741455, 15))}
RUN_MIN = 128                     # kMsmRunMin (msm.h)
RUN_MINS = (16, 32, 64, 128, 256)


def auto_window(group, n):
    for below, c in AUTO_WINDOW[group]:
        if n < below:
            return c
    return 16


def run_cap(n, c, run_min):
    """msm.h msm_run_cap_default with run_min for kMsmRunMin"""
    return max(run_min, 2 * -(-n // (1 << (c - 1))))


def windows(c):
    return 254 // c + 1


def bucket_products(n, c, group="g1"):
    """Fq products of the bucket path by count: n additions per window into the buckets,
    two per bucket and a (c-1)-bit double-and-add per segment in the reduction, the
    segment tree, Horner over the windows."""
    ADD, DBL = OPS[group]
    w, nb = windows(c), 1 << (c - 1)
    nseg = (nb + SEGMENT - 1) // SEGMENT
    adds = n * w + 2 * nb * w + nseg * w * c + (nseg - 1) * w + (w - 1)
    dbls = nseg * w * (c - 1) + (w - 1) * c
    return ADD * adds + DBL * dbls


def small_products(n, group="g1"):
    """254 doublings and 127 additions per term on average, n - 1 additions in the tree"""
    ADD, DBL = OPS[group]
    return n * (254 * DBL + 127 * ADD) + (n - 1) * ADD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=("g1", "g2"), default="g1")
    ap.add_argument("--sizes", default=None,
                    help="default: 1,16,128,512,2^10 .. 2^20; with --basis 1,2^10,2^12,2^14,2^16 .. 2^20")
    ap.add_argument("--windows", default="8,9,10,11,12,13,14,15,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skew", type=int, default=1 << 18)
    ap.add_argument("--run-cap", action="store_true", help="sweep the run cap and the skew patterns instead of the window")
    ap.add_argument("--skew-reps", type=int, default=10)
    ap.add_argument("--basis", action="store_true", help="bn_g1_msm against bn_g1_msm_basis over a fixed basis (--group g2: the G2 forms)")
    ap.add_argument("--basis-windows", default="", help="widths of the basis form; empty: its default and the two on either side")
    ap.add_argument("--basis-many", action="store_true", help="bn_g1_msm_basis_many against a loop of bn_g1_msm_basis calls")
    ap.add_argument("--many-m", default="2,8,32,128")
    ap.add_argument("--many-shapes", default="9x65536", help="further shapes m x n; empty: none")
    ap.add_argument("--many-set-keys", default="", help="bounds on S * nkeys to sweep, e.g. 2097152,4194304,8388608")
    ap.add_argument("--many-loop-only", action="store_true")
    ap.add_argument("--many-only", action="store_true", help="the batched form alone, unchecked (a profiler run of its own)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from substrate_bn import Context, _native, synth

    grp = args.group
    words = {"g1": 12, "g2": 24}[grp]

    def emit(rec):
        if grp != "g1":
            rec = dict({"group": grp}, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    dev = torch.device("cuda", 0)
    ctx, dctx = Context(0), Context(0)
    if args.sizes:
        sizes = [int(s) for s in args.sizes.split(",")]
    elif args.basis_many:
        sizes = [1 << e for e in (10, 12, 14, 16, 18)]
    elif args.basis:
        sizes = [1, 1 << 10, 1 << 12, 1 << 14] + [1 << e for e in range(16, 21)]
    else:
        sizes = [1, 16, 128, 512] + [1 << e for e in range(10, 21)]
    cs = [int(c) for c in args.windows.split(",")]
    many_shapes = [tuple(int(v) for v in t.split("x")) for t in args.many_shapes.split(",") if t] if args.basis_many else []
    nmax = max(sizes + [n for _, n in many_shapes]) if args.basis_many else max(sizes + [args.skew])
    s = synth.fr_images_raw(nmax, 0x6d736d31)
    k = synth.fr_images_raw(nmax, 0x6d736d32, lo=0)
    one = synth.g1_one_image() if grp == "g1" else synth.g2_one_image()
    gen = torch.from_numpy(np.tile(one.view(np.int64), (nmax, 1))).to(dev)
    sd = torch.from_numpy(s.view(np.int64)).to(dev)
    K = torch.from_numpy(k.view(np.int64)).to(dev)
    P = torch.empty((nmax, words), dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    torch.cuda.synchronize(dev)
    mul_many = ctx.g1_mul_many_dev if grp == "g1" else ctx.g2_mul_many_dev
    mul_many(gen.data_ptr(), sd.data_ptr(), nmax, P.data_ptr(), sh)
    torch.cuda.synchronize(dev)
    out = torch.zeros(words, dtype=torch.int64, device=dev)

    def setup(name):
        """-> the context to call for form `name`, set up for it"""
        if name == "default":
            return dctx
        if name == "small":
            ctx.set_msm_window(0)
            ctx.set_msm_min(nmax + 1)
        else:
            ctx.set_msm_min(0)
            ctx.set_msm_window(int(name[2:]))
        return ctx

    def reserve(c, n):
        if grp == "g1":
            c.msm_reserve(n)
        else:
            c.g2_msm_reserve(n)

    def setup_cap(name, n):
        """the same for the forms of --run-cap"""
        if name == "small":
            return setup("small")
        ctx.set_msm_min(0)
        ctx.set_msm_window(0)
        if name in ("unsplit", "default", "split"):
            ctx.set_msm_run_max(_native.MSM_RUN_UNSPLIT if name == "unsplit" else 0)
        else:
            ctx.set_msm_run_max(run_cap(n, auto_window(grp, n), int(name[3:])))
        return ctx

    def run(name, n, kd, timed):
        c = setup_cap(name, n) if args.run_cap else setup(name)
        if not timed:
            reserve(c, n)
        msm_dev = c.g1_msm_dev if grp == "g1" else c.g2_msm_dev
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            msm_dev(P.data_ptr(), kd.data_ptr(), n, out.data_ptr(), sh)
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), out.cpu().numpy().view(np.uint64).copy()

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    if args.basis_many:
        shapes = [(m, n) for n in sizes for m in (int(v) for v in args.many_m.split(","))] + many_shapes
        basis_many_sweep(args, shapes, dctx, P, stream, stats, emit, dev)
        return
    if args.basis:
        basis_sweep(args, grp, sizes, dctx, P, K, k, out, stream, stats, emit, dev)
        return
    if args.run_cap:
        run_cap_sweep(args, grp, sizes, run, stats, emit, k, K, dev)
        return
    forms = ["small"] + ["c=%d" % c for c in cs] + ["default"]
    for n in sizes:
        want = None
        for f in forms:  # warm-up (allocates) and the agreement check
            _, got = run(f, n, K, False)
            if want is None:
                want = got
            elif not np.array_equal(got, want):
                print("MISMATCH at n=%d: %s differs from the small path" % (n, f), file=sys.stderr)
                sys.exit(1)
        times = {f: [] for f in forms}
        for _ in range(args.reps):
            for f in forms:
                times[f].append(run(f, n, K, True)[0])
        rec = {"n": n, "reps": args.reps, "small": stats(times["small"]), "default": stats(times["default"])}
        rec["small"]["frac"] = round(small_products(n, grp) * 128 / (rec["small"]["median_ms"] * 1e-3) / PEAK_MAD32, 4)
        best = None
        for c in cs:
            st = stats(times["c=%d" % c])
            st["frac"] = round(bucket_products(n, c, grp) * 128 / (st["median_ms"] * 1e-3) / PEAK_MAD32, 4)
            rec["c=%d" % c] = st
            if best is None or st["median_ms"] < rec["c=%d" % best]["median_ms"]:
                best = c
        rec["best_c"] = best
        rec["small_over_best"] = round(rec["small"]["median_ms"] / rec["c=%d" % best]["median_ms"], 3)
        rec["small_spread_ms"] = round(rec["small"]["max_ms"] - rec["small"]["min_ms"], 4)
        emit(rec)
    if args.skew:
        n = args.skew
        ke = torch.from_numpy(np.tile(k[7].view(np.int64), (n, 1))).to(dev)
        torch.cuda.synchronize(dev)
        _, want = run("small", n, ke, False)
        dctx.set_msm_min(0)  # the bucket path at the table's window, whatever the threshold
        reserve(dctx, n)
        ms, got = run("default", n, ke, True)
        if not np.array_equal(got, want):
            print("MISMATCH on the all-equal batch", file=sys.stderr)
            sys.exit(1)
        ms_small, _ = run("small", n, ke, True)
        emit({"skew_all_equal_n": n, "bucket_ms": round(ms, 3), "small_ms": round(ms_small, 3), "reps": 1})


def run_cap_sweep(args, grp, sizes, run, stats, emit, k, K, dev):
    import torch

    forms = ["unsplit", "default"] + ["L0=%d" % m for m in RUN_MINS]
    for n in sizes:
        want = None
        for f in forms:  # warm-up (allocates) and the agreement check
            _, got = run(f, n, K, False)
            if want is None:
                want = got
            elif not np.array_equal(got, want):
                print("MISMATCH at n=%d: %s differs from unsplit" % (n, f), file=sys.stderr)
                sys.exit(1)
        times = {f: [] for f in forms}
        for _ in range(args.reps):
            for f in forms:
                times[f].append(run(f, n, K, True)[0])
        c = auto_window(grp, n)
        rec = {"n": n, "reps": args.reps, "c": c, "default_cap": run_cap(n, c, RUN_MIN)}
        for f in forms:
            rec[f] = stats(times[f])
        rec["default_in_unsplit_spread"] = rec["unsplit"]["min_ms"] <= rec["default"]["median_ms"] <= rec["unsplit"]["max_ms"]
        rec["default_over_unsplit"] = round(rec["default"]["median_ms"] / rec["unsplit"]["median_ms"], 4)
        emit(rec)
    if not args.skew:
        return
    n = args.skew
    for name, kv in skew_patterns(k, n).items():
        kd = torch.from_numpy(np.ascontiguousarray(kv).view(np.int64)).to(dev)
        torch.cuda.synchronize(dev)
        _, want = run("small", n, kd, False)
        _, got = run("split", n, kd, False)
        if not np.array_equal(got, want):
            print("MISMATCH on %s: split differs from the small path" % name, file=sys.stderr)
            sys.exit(1)
        # the split form's warm-up has allocated all unsplit needs; its one repetition is also its check
        ms_unsplit, got = run("unsplit", n, kd, True)
        if not np.array_equal(got, want):
            print("MISMATCH on %s: unsplit differs from the small path" % name, file=sys.stderr)
            sys.exit(1)
        times = {"split": [], "small": []}
        for _ in range(args.skew_reps):
            for f in times:
                times[f].append(run(f, n, kd, True)[0])
        rec = {"skew": name, "n": n, "c": auto_window(grp, n), "unsplit_ms": round(ms_unsplit, 3), "unsplit_reps": 1,
               "reps": args.skew_reps, "split": stats(times["split"]), "small": stats(times["small"])}
        rec["split_beats_small"] = rec["split"]["median_ms"] < rec["small"]["median_ms"]
        emit(rec)


def skew_patterns(k, n):
    """the four skewed scalar patterns of --run-cap and --basis: {name: (n, 4) images}"""
    from oracle import oracle as O
    one, minus_one = O.canon_to_mont_array([1, O.R - 1], O.FR).reshape(2, 4)
    uni = k[:n]
    pats = {"all_equal": np.tile(k[7], (n, 1)), "all_one": np.tile(one, (n, 1))}
    half = uni.copy()
    half[0::2] = one
    pats["half_one"] = half
    pct = uni.copy()
    pct[0::100] = minus_one
    pats["one_pct_minus_one"] = pct
    return pats


def basis_sweep(args, grp, sizes, dctx, P, K, k, out, stream, stats, emit, dev):
    import torch

    from substrate_bn import _native
    sh = stream.cuda_stream
    # the group's calls: bn_<grp>_msm_dev, its reserve call, and the basis form's
    msm_dev = getattr(dctx, grp + "_msm_dev")
    msm_reserve = dctx.msm_reserve if grp == "g1" else dctx.g2_msm_reserve
    basis_prepare_dev, basis_destroy = getattr(dctx, grp + "_basis_prepare_dev"), getattr(dctx, grp + "_basis_destroy")
    basis_window, basis_reserve = getattr(dctx, grp + "_basis_window"), getattr(dctx, grp + "_msm_basis_reserve")
    msm_basis_dev, table_bytes = getattr(dctx, grp + "_msm_basis_dev"), getattr(_native, grp + "_basis_table_bytes")

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            call()
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), out.cpu().numpy().view(np.uint64).copy()

    def prepared(n, c):
        """-> a handle over P[:n] at width c (0: the default) and the device time of its build,
        the second of two (the first warms up)"""
        made = []
        for _ in range(2):
            if made:
                basis_destroy(made.pop())
            ms, _ = timed(lambda: made.append(basis_prepare_dev(P.data_ptr(), n, c, sh)))
        return made[0], ms

    def compare(n, kd, handles, reps, what):
        """-> {form: stats} of the group's single MSM and the basis form at every width over the scalars kd,
        after a warm-up of every form that is also the agreement check"""
        forms = {"msm": lambda: msm_dev(P.data_ptr(), kd.data_ptr(), n, out.data_ptr(), sh)}
        for c, h in handles.items():
            forms["basis c=%d" % c] = lambda h=h: msm_basis_dev(h, kd.data_ptr(), n, out.data_ptr(), sh)
        msm_reserve(n)
        for h in handles.values():
            basis_reserve(h, n)
        want = None
        for f, call in forms.items():
            _, got = timed(call)
            if want is None:
                want = got
            elif not np.array_equal(got, want):
                print("MISMATCH at %s: %s differs from bn_%s_msm" % (what, f, grp), file=sys.stderr)
                sys.exit(1)
        times = {f: [] for f in forms}
        for _ in range(reps):
            for f, call in forms.items():
                times[f].append(timed(call)[0])
        return {f: stats(ts) for f, ts in times.items()}

    def verdict(rec, c0):
        a, b = rec["msm"], rec["basis c=%d" % c0]
        spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        rec["msm_over_basis"] = round(a["median_ms"] / b["median_ms"], 3)
        rec["spread_ms"] = round(spread, 4)
        rec["gain_outside_spread"] = a["median_ms"] - b["median_ms"] > spread
        rec["basis_not_slower"] = b["median_ms"] <= a["median_ms"]

    def sized(n, body):
        """body(c0, {c: handle}, {width: prepare time and table bytes}) over handles of n bases"""
        h0, ms0 = prepared(n, 0)
        c0 = basis_window(h0)
        handles, prep = {c0: h0}, {c0: ms0}
        try:
            others = [int(c) for c in args.basis_windows.split(",")] if args.basis_windows else [c0 - 1, c0 + 1]
            for c in others:
                if 2 <= c <= 16 and c not in handles:
                    handles[c], prep[c] = prepared(n, c)
            handles = dict(sorted(handles.items()))
            body(c0, handles, {"c=%d" % c: {"prepare_ms": round(prep[c], 3), "table_bytes": table_bytes(n, c)}
                               for c in handles})
        finally:
            for h in handles.values():
                basis_destroy(h)

    for n in sizes:
        def body(c0, handles, prep, n=n):
            rec = {"n": n, "reps": args.reps, "basis_default_c": c0, "msm_auto_c": auto_window(grp, n), "prepare": prep}
            rec.update(compare(n, K, handles, args.reps, "n=%d" % n))
            verdict(rec, c0)
            rec["best_basis_c"] = min(handles, key=lambda c: rec["basis c=%d" % c]["median_ms"])
            emit(rec)
        sized(n, body)
    if not args.skew:
        return
    n = args.skew

    def body(c0, handles, prep):
        for name, kv in skew_patterns(k, n).items():
            kd = torch.from_numpy(np.ascontiguousarray(kv).view(np.int64)).to(dev)
            torch.cuda.synchronize(dev)
            rec = {"skew": name, "n": n, "reps": args.skew_reps, "basis_default_c": c0, "msm_auto_c": auto_window(grp, n)}
            rec.update(compare(n, kd, {c0: handles[c0]}, args.skew_reps, name))
            verdict(rec, c0)
            emit(rec)
    sized(n, body)


def basis_many_sweep(args, shapes, ctx, P, stream, stats, emit, dev):
    import torch

    sh = stream.cuda_stream
    set_keys = [int(v) for v in args.many_set_keys.split(",") if v]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            call()
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def scalars(m, n):
        """m x n Fr images on the device: uniform 253-bit values (every value below r is an image)"""
        g = torch.Generator(device=dev)
        g.manual_seed(0x6d616e79 + m * 31 + n)
        k = torch.randint(-2 ** 63, 2 ** 63 - 1, (m * n, 4), dtype=torch.int64, device=dev, generator=g)
        k[:, 3] &= (1 << 61) - 1
        return k

    handles = {}
    try:
        for m, n in shapes:
            rec = {"m": m, "n": n, "reps": args.reps}
            try:
                if n not in handles:
                    for h in handles.values():
                        ctx.g1_basis_destroy(h)
                    handles.clear()
                    handles[n] = ctx.g1_basis_prepare_dev(P.data_ptr(), n, 0, sh)
                h = handles[n]
                c = ctx.g1_basis_window(h)
                nkeys = (254 // c + 1) << (c - 1)
                rec["c"] = c
                K = scalars(m, n)
                out_many = torch.zeros((m, 12), dtype=torch.int64, device=dev)
                out_loop = torch.zeros((m, 12), dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                ctx.g1_msm_basis_reserve(h, n)
                if not args.many_loop_only:
                    ctx.set_msm_basis_many_set(max(1, max(set_keys) // nkeys) if set_keys else 0)
                    ctx.g1_msm_basis_many_reserve(h, m, n)
            except Exception as e:  # the scalars, the table or the workspace do not fit
                rec["skipped"] = str(e)[:200]
                emit(rec)
                continue

            def loop():
                for j in range(m):
                    ctx.g1_msm_basis_dev(h, K.data_ptr() + j * n * 32, n, out_loop.data_ptr() + j * 96, sh)

            def many():
                ctx.g1_msm_basis_many_dev(h, K.data_ptr(), n, m, n, out_many.data_ptr(), 1, sh)

            forms = {} if args.many_only else {"loop": loop}
            if args.many_loop_only:
                pass
            elif set_keys:
                for b in set_keys:
                    def f(b=b):
                        ctx.set_msm_basis_many_set(max(1, b // nkeys))
                        many()
                    forms["many keys=%d" % b] = f
                rec["S"] = {"keys=%d" % b: min(m, max(1, b // nkeys)) for b in set_keys}
            else:
                forms["many"] = many
                rec["S"] = min(m, max(1, min((1 << 23) // nkeys, (2 ** 31 - 1) // (n * (254 // c + 1)))))
            for f, call in forms.items():  # the warm-up, which is also the byte-equality check
                out_many.zero_()
                timed(call)
                if f != "loop" and "loop" in forms and not torch.equal(out_many, out_loop):
                    print("MISMATCH at m=%d n=%d: %s differs from the loop of single calls" % (m, n, f), file=sys.stderr)
                    sys.exit(1)
            times = {f: [] for f in forms}
            for _ in range(args.reps):
                for f, call in forms.items():
                    times[f].append(timed(call))
            for f, ts in times.items():
                rec[f] = stats(ts)
            a = rec.get("loop")
            for f in forms:
                if f == "loop" or a is None:
                    continue
                b = rec[f]
                spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
                b["loop_over_many"] = round(a["median_ms"] / b["median_ms"], 3)
                b["spread_ms"] = round(spread, 4)
                b["gain_outside_spread"] = a["median_ms"] - b["median_ms"] > spread
            emit(rec)
            del K, out_many, out_loop
    finally:
        for h in handles.values():
            ctx.g1_basis_destroy(h)


if __name__ == "__main__":
    main()
