#!/usr/bin/env python3
"""Device time of bn_g1_msm_prepared_many_dev per shape (m MSMs over k shared bases) with
the method of tools/msm_bench.py: HBM-resident inputs, the workspace reserved, a warm-up of
every form, --reps repetitions per form alternating in one process, torch events on the
launch stream, median and min-max.  Forms:
  c=K        the new call on a table of width K, lanes per output automatic
  c=K,L=N    at the fastest K, every allowed number of lanes per output
  default    the new call on a default handle of a context with untouched settings
  baseline   what a caller composes without it: bn_g1_mul_many_dev over m * k terms with the
             bases replicated (base major, so that the tree adds contiguous halves),
             ceil(log2 k) bn_g1_add_many_dev calls, bn_g1_normalize_many_dev
  singles    m <= 2^10 only: m bn_g1_msm_dev calls of k terms (--single-reps repetitions)
Before a shape is timed every form must return the same m * 96 bytes, else the script
exits non-zero.  One JSON line per shape; before them one line per (k, c) with the time of
bn_g1_bases_prepare_dev; after them (--groth16 M) one end-to-end line for M Groth16-shaped
verifications: vk_x of 17 terms written at stride 4 into the p array of
bn_pairing_batch_prepared_many_dev, then that call, against the baseline composition (and
the strided copy it needs) in front of the same call.  `products` is the derived count of
Fq products per output: k * W(c) mixed additions of 11 and two loads of 1 each, the tree of
16 per lane beyond the first, one normalization; for the baseline 254 doublings of 7 and
127 additions of 16 per term, k - 1 additions of 16 and the normalization.
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

NORMALIZE = 400   # an Fq inversion by Fermat (about 254 squarings and 130 products) and 4 products
LANES = [1, 2, 4, 8, 16, 32, 64]


def windows(c):
    return 254 // c + 1


def auto_lanes(m, k, c):
    """msm_fixed_auto_lanes (csrc/msm_fixed.h)"""
    pairs = k * windows(c)
    target = 1 << 17 if pairs < 832 else 1 << 19
    lanes = 1
    while lanes < 64 and m * lanes < target and 8 * lanes <= pairs:
        lanes *= 2
    return lanes


def prepared_products(k, c, lanes):
    return k * windows(c) * 13 + (lanes - 1) * 16 + NORMALIZE


def baseline_products(k):
    return k * (254 * 7 + 127 * 16) + (k - 1) * 16 + NORMALIZE


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="1024,4096,16384,65536")
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--windows", default="4,5,6,7,8,9,10")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single-reps", type=int, default=3)
    ap.add_argument("--groth16", type=int, default=1 << 14)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from substrate_bn import Context, _native, synth

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    dev = torch.device("cuda", 0)
    ctx, dctx = Context(0), Context(0)
    ms = [int(x) for x in args.ms.split(",")]
    ks = [int(x) for x in args.ks.split(",")]
    cs = [int(x) for x in args.windows.split(",")]
    kmax = max(ks + [17])
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    # kmax bases s_b * G1::one() (Jacobian images) and the scalars of the largest shape
    gen = to_dev(np.tile(synth.g1_one_image(), (kmax, 1)))
    sb = to_dev(synth.fr_images_raw(kmax, 0x70726531))
    BASES = torch.empty((kmax, 12), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_many_dev(gen.data_ptr(), sb.data_ptr(), kmax, BASES.data_ptr(), sh)
    torch.cuda.synchronize(dev)
    scal = synth.fr_images_raw(max(ms) * max(ks), 0x70726532, lo=0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    # ---- prepare time per (k, c); the handles are kept for the sweep
    handles = {}
    for k in ks:
        for c in cs:
            ts = []
            for _ in range(3):
                if (k, c) in handles:
                    ctx.g1_prepared_destroy(handles[(k, c)])
                box = {}
                ts.append(timed(lambda: box.update(h=ctx.g1_bases_prepare_dev(BASES.data_ptr(), k, c, sh))))
                handles[(k, c)] = box["h"]
            emit({"prepare": {"k": k, "c": c}, "table_bytes": int(_native.g1_prepared_table_bytes(k, c)),
                  **stats(ts), "reps": 3})
    dhandles = {k: dctx.g1_bases_prepare_dev(BASES.data_ptr(), k, 0, sh) for k in ks}
    torch.cuda.synchronize(dev)

    for m in ms:
        for k in ks:
            K = to_dev(scal[:m * k])                                   # (m, k) row major
            Kt = to_dev(scal[:m * k].reshape(m, k, 4).transpose(1, 0, 2))   # (k, m): the baseline's layout
            REP = BASES[:k].repeat_interleave(m, dim=0).contiguous()   # base b at rows b * m .. b * m + m - 1
            T = torch.empty((m * k, 12), dtype=torch.int64, device=dev)
            OUT = torch.zeros((m, 12), dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)
            ctx.msm_reserve(max(m * 64, k))
            dctx.msm_reserve(max(m * 64, k))

            def new_call(c, lanes):
                def fn():
                    ctx.set_msm_prepared_lanes(lanes)
                    ctx.g1_msm_prepared_many_dev(handles[(k, c)], K.data_ptr(), m, OUT.data_ptr(), 1, sh)
                return fn

            def default_call():
                dctx.g1_msm_prepared_many_dev(dhandles[k], K.data_ptr(), m, OUT.data_ptr(), 1, sh)

            def baseline():
                ctx.g1_mul_many_dev(REP.data_ptr(), Kt.data_ptr(), m * k, T.data_ptr(), sh)
                n = k
                while n > 1:
                    h = (n + 1) // 2
                    ctx.group_op_many_dev("g1", "add", T.data_ptr(), T.data_ptr() + h * m * 96, (n - h) * m,
                                          T.data_ptr(), sh)
                    n = h
                ctx.group_op_many_dev("g1", "normalize", T.data_ptr(), None, m, OUT.data_ptr(), sh)

            def singles():
                for j in range(m):
                    dctx.g1_msm_dev(BASES.data_ptr(), K.data_ptr() + j * k * 32, k, OUT.data_ptr() + j * 96, sh)

            def result(fn):
                OUT.zero_()
                torch.cuda.synchronize(dev)
                t = timed(fn)
                return t, OUT.cpu().numpy().view(np.uint64).copy()

            forms = {"baseline": baseline, "default": default_call}
            for c in cs:
                forms["c=%d" % c] = new_call(c, 0)
            if m <= 1024:
                forms["singles"] = singles
            want = None
            for name, fn in forms.items():  # warm-up and the agreement check
                _, got = result(fn)
                if want is None:
                    want = got
                elif not np.array_equal(got, want):
                    print("MISMATCH at m=%d k=%d: %s differs from the baseline" % (m, k, name), file=sys.stderr)
                    sys.exit(1)
            times = {name: [] for name in forms}
            for r in range(args.reps):
                for name, fn in forms.items():
                    if name != "singles" or r < args.single_reps:
                        times[name].append(timed(fn))
            rec = {"m": m, "k": k, "reps": args.reps}
            for name in forms:
                rec[name] = stats(times[name])
            best = min(cs, key=lambda c: rec["c=%d" % c]["median_ms"])
            rec["best_c"] = best
            rec["auto_lanes"] = {str(c): auto_lanes(m, k, c) for c in cs}
            # every allowed number of lanes at the fastest width
            lane_forms = {"c=%d,L=%d" % (best, n): new_call(best, n) for n in LANES}
            for name, fn in lane_forms.items():
                _, got = result(fn)
                if not np.array_equal(got, want):
                    print("MISMATCH at m=%d k=%d: %s differs from the baseline" % (m, k, name), file=sys.stderr)
                    sys.exit(1)
            ltimes = {name: [] for name in lane_forms}
            for _ in range(args.reps):
                for name, fn in lane_forms.items():
                    ltimes[name].append(timed(fn))
            for name in lane_forms:
                rec[name] = stats(ltimes[name])
            rec["best_lanes"] = min(LANES, key=lambda n: rec["c=%d,L=%d" % (best, n)]["median_ms"])
            rec["baseline_over_best"] = round(rec["baseline"]["median_ms"] / rec["c=%d" % best]["median_ms"], 2)
            rec["baseline_over_default"] = round(rec["baseline"]["median_ms"] / rec["default"]["median_ms"], 2)
            rec["products"] = {"baseline": baseline_products(k),
                               "best": prepared_products(k, best, auto_lanes(m, k, best))}
            rec["derived_ratio"] = round(rec["products"]["baseline"] / rec["products"]["best"], 2)
            ctx.set_msm_prepared_lanes(0)
            emit(rec)
            del K, Kt, REP, T, OUT

    if args.groth16:
        m, k = args.groth16, 17
        p, q, _, _ = synth_pairs(synth, ctx, m, dev, sh, torch)
        g2h = dctx.g2_prepare_dev(q[:3].data_ptr(), 3, sh)
        h = dctx.g1_bases_prepare_dev(BASES.data_ptr(), k, 0, sh)
        K = to_dev(synth.fr_images_raw(m * k, 0x70726533, lo=0))
        Kt = to_dev(synth.fr_images_raw(m * k, 0x70726533, lo=0).reshape(m, k, 4).transpose(1, 0, 2))
        REP = BASES[:k].repeat_interleave(m, dim=0).contiguous()
        T = torch.empty((m * k, 12), dtype=torch.int64, device=dev)
        V = torch.zeros((m, 12), dtype=torch.int64, device=dev)
        P = p[:4 * m].clone()
        QF = q[3:3 + m].contiguous()
        GT = torch.zeros((m, 48), dtype=torch.int64, device=dev)
        qidx = np.tile(np.array([0, 1, 0xFFFFFFFF, 2], np.uint32), m)
        off = np.arange(0, 4 * m + 1, 4).astype(np.uintp)
        dctx.reserve(4 * m)
        dctx.msm_reserve(max(m * 64, m * k))
        torch.cuda.synchronize(dev)

        def products():
            dctx.pairing_batch_prepared_many_dev(P.data_ptr(), QF.data_ptr(), g2h, qidx, off, GT.data_ptr(), sh)

        def with_prepared():
            dctx.g1_msm_prepared_many_dev(h, K.data_ptr(), m, P.data_ptr(), 4, sh)
            products()

        def with_baseline():
            dctx.g1_mul_many_dev(REP.data_ptr(), Kt.data_ptr(), m * k, T.data_ptr(), sh)
            n = k
            while n > 1:
                hh = (n + 1) // 2
                dctx.group_op_many_dev("g1", "add", T.data_ptr(), T.data_ptr() + hh * m * 96, (n - hh) * m,
                                       T.data_ptr(), sh)
                n = hh
            dctx.group_op_many_dev("g1", "normalize", T.data_ptr(), None, m, V.data_ptr(), sh)
            with torch.cuda.stream(stream):
                P.view(m, 4, 12)[:, 0].copy_(V)
            products()

        forms = {"pairing_products_alone": products, "with_prepared_msm": with_prepared, "with_baseline": with_baseline}
        outs = {}
        for name, fn in forms.items():
            timed(fn)
            outs[name] = GT.cpu().numpy().copy()
        if not np.array_equal(outs["with_prepared_msm"], outs["with_baseline"]):
            print("MISMATCH in the Groth16-shaped run", file=sys.stderr)
            sys.exit(1)
        times = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, fn in forms.items():
                times[name].append(timed(fn))
        emit({"groth16": m, "k": k, "reps": args.reps, **{name: stats(times[name]) for name in forms}})


def synth_pairs(synth, ctx, m, dev, sh, torch):
    """4 m G1 points and 3 + m G2 points on the device: random multiples of the generators"""
    n1, n2 = 4 * m, 3 + m
    g1 = torch.from_numpy(np.tile(synth.g1_one_image().view(np.int64), (n1, 1))).to(dev)
    g2 = torch.from_numpy(np.tile(synth.g2_one_image().view(np.int64), (n2, 1))).to(dev)
    s1 = torch.from_numpy(synth.fr_images_raw(n1, 0x70726534).view(np.int64)).to(dev)
    s2 = torch.from_numpy(synth.fr_images_raw(n2, 0x70726535).view(np.int64)).to(dev)
    p = torch.empty((n1, 12), dtype=torch.int64, device=dev)
    q = torch.empty((n2, 24), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_many_dev(g1.data_ptr(), s1.data_ptr(), n1, p.data_ptr(), sh)
    ctx.g2_mul_many_dev(g2.data_ptr(), s2.data_ptr(), n2, q.data_ptr(), sh)
    torch.cuda.synchronize(dev)
    return p, q, s1, s2


if __name__ == "__main__":
    main()
