#!/usr/bin/env python3
"""Device time of bn_g1_msm_many_dev per shape (m MSMs of `len` fresh terms each) with the
method of tools/msm_prepared_bench.py: HBM-resident inputs, the workspace reserved, a
warm-up of every form, --reps repetitions per form alternating in one process, torch events
on the launch stream, median and min-max.  Forms:
  c=K,T=N    the new call at window width K with N terms per unit forced
  default    the new call on a context with untouched settings
  baseline   what a caller composes without it: bn_g1_mul_many_dev over all terms laid out
             term major (so that the tree adds contiguous halves), ceil(log2 len)
             bn_g1_add_many_dev calls, bn_g1_normalize_many_dev.  For the ragged shape the
             segments are padded to the longest with zero scalars, which is what such a
             caller has to do.
  singles    m <= 2^10 only: m bn_g1_msm_dev calls (--single-reps repetitions)
  alone      --long only: the new call with the max below the segment length, so that every
             segment runs on bn_g1_msm's path
Before a shape is timed every form must return the same m * 96 bytes, else the script exits
non-zero.  One JSON line per shape; then (--ragged M) one ragged call with lengths 1 .. 64
cycling, (--long M) M segments of 2,048 terms packed against alone, and (--kzg M) one
end-to-end line for M KZG-shaped verifications: two MSMs of 16 terms each written at stride 1
into the p array of bn_pairing_batch_prepared_many_dev over two prepared G2 points, then that
call, with the new call in front and with the composition in front.  `products` is the
derived count of Fq products per term: for the new call W(c) (1 - 2^-c) additions of 16, the
multiples (a doubling of 7 and 2^(c-1) - 2 additions of 14) and 254 doublings of 7 shared by
the T terms of a unit; for the baseline 254 doublings of 7 and 127 additions of 16.
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

BASELINE_PRODUCTS = 254 * 7 + 127 * 16


def windows(c):
    return 254 // c + 1


def many_products(c, unit):
    return round(windows(c) * (1 - 2.0 ** -c) * 16 + 7 + ((1 << (c - 1)) - 2) * 14 + 254 * 7 / unit, 1)


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="1024,4096,16384,65536")
    ap.add_argument("--lens", default="2,8,32,256")
    ap.add_argument("--windows", default="3,4,5,6")
    ap.add_argument("--units", default="1,2,4,8,16,32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--single-reps", type=int, default=3)
    ap.add_argument("--max-terms", type=int, default=1 << 24, help="skip shapes of more terms")
    ap.add_argument("--ragged", type=int, default=1 << 14)
    ap.add_argument("--long", type=int, default=1 << 10)
    ap.add_argument("--kzg", type=int, default=1 << 14)
    ap.add_argument("--long-reps", type=int, default=3, help="repetitions of the --long shape (its alone form takes seconds)")
    ap.add_argument("--chunk", type=int, default=0, help="bn_set_msm_many_chunk for the forced forms; 0: the default")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    from substrate_bn import Context, synth

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    dev = torch.device("cuda", 0)
    ctx, dctx = Context(0), Context(0)
    ms = [int(x) for x in args.ms.split(",") if x]
    lens = [int(x) for x in args.lens.split(",") if x]
    cs = [int(x) for x in args.windows.split(",") if x]
    units = [int(x) for x in args.units.split(",") if x]
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream
    shapes = [(m, ln) for m in ms for ln in lens if m * ln <= args.max_terms]
    npool = max([m * ln for m, ln in shapes] + [args.ragged * 64, args.long * 2048, args.kzg * 32, 1])

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    # the pool: npool points s_i * G1::one() (Jacobian images) and npool scalars
    gen = to_dev(np.tile(synth.g1_one_image(), (npool, 1)))
    sb = to_dev(synth.fr_images_raw(npool, 0x6d616e31))
    PTS = torch.empty((npool, 12), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_many_dev(gen.data_ptr(), sb.data_ptr(), npool, PTS.data_ptr(), sh)
    torch.cuda.synchronize(dev)
    del gen, sb
    SCAL = to_dev(synth.fr_images_raw(npool, 0x6d616e32, lo=0)).view(npool, 4)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def settings(c, unit, max_terms=4096):
        ctx.set_msm_many_window(c)
        ctx.set_msm_many_unit(unit)
        ctx.set_msm_many_max(max_terms)
        ctx.set_msm_many_chunk(args.chunk)

    def run_shape(tag, lengths_of, m, sweep, extra=None, reps=None):
        """lengths_of(m) -> the m segment lengths; sweep: the (c, unit) pairs to time"""
        lengths = lengths_of(m)
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uintp)
        n, lmax = int(off[-1]), int(max(lengths))
        P, K = PTS[:n], SCAL[:n]
        OUT = torch.zeros((m, 12), dtype=torch.int64, device=dev)
        # the baseline's layout: term i of segment j at row i * m + j, padded to lmax terms
        idx = np.zeros((lmax, m), np.int64)
        live = np.zeros((lmax, m), bool)
        for i in range(lmax):
            has = lengths > i
            idx[i, has] = off[:-1][has].astype(np.int64) + i
            live[i] = has
        gi = torch.from_numpy(idx.reshape(-1)).to(dev)
        REP = P[gi].contiguous()
        Kt = (K[gi] * torch.from_numpy(live.reshape(-1).astype(np.int64)).to(dev)[:, None]).contiguous()
        T = torch.empty((lmax * m, 12), dtype=torch.int64, device=dev)
        del gi
        torch.cuda.synchronize(dev)
        for c in (ctx, dctx):
            c.g1_msm_many_reserve(n, m)
            c.msm_reserve(max(lmax, 1))

        def new_call(c, unit, max_terms=4096):
            def fn():
                settings(c, unit, max_terms)
                ctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), off, OUT.data_ptr(), 1, sh)
            return fn

        def default_call():
            dctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), off, OUT.data_ptr(), 1, sh)

        def baseline():
            ctx.g1_mul_many_dev(REP.data_ptr(), Kt.data_ptr(), lmax * m, T.data_ptr(), sh)
            k = lmax
            while k > 1:
                h = (k + 1) // 2
                ctx.group_op_many_dev("g1", "add", T.data_ptr(), T.data_ptr() + h * m * 96, (k - h) * m, T.data_ptr(), sh)
                k = h
            ctx.group_op_many_dev("g1", "normalize", T.data_ptr(), None, m, OUT.data_ptr(), sh)

        def singles():
            for j in range(m):
                dctx.g1_msm_dev(P.data_ptr() + int(off[j]) * 96, K.data_ptr() + int(off[j]) * 32, int(lengths[j]),
                                OUT.data_ptr() + j * 96, sh)

        forms = {"baseline": baseline, "default": default_call}
        for c, unit in sweep:
            forms["c=%d,T=%d" % (c, unit)] = new_call(c, unit)
        if extra:
            for name, (c, unit, max_terms) in extra.items():
                forms[name] = new_call(c, unit, max_terms)
        if m <= 1024 and args.single_reps:
            forms["singles"] = singles
        want = None
        for name, fn in forms.items():  # warm-up and the agreement check
            OUT.zero_()
            torch.cuda.synchronize(dev)
            timed(fn)
            got = OUT.cpu().numpy().view(np.uint64).copy()
            if want is None:
                want = got
            elif not np.array_equal(got, want):
                print("MISMATCH at %s m=%d: %s differs from the baseline" % (tag, m, name), file=sys.stderr)
                sys.exit(1)
        reps = reps or args.reps
        times = {name: [] for name in forms}
        for r in range(reps):
            for name, fn in forms.items():
                if name != "singles" or r < args.single_reps:
                    times[name].append(timed(fn))
        rec = {"shape": tag, "m": m, "terms": n, "reps": reps, "chunk": args.chunk}
        for name in forms:
            rec[name] = stats(times[name])
        if sweep:
            best = min(sweep, key=lambda cu: rec["c=%d,T=%d" % cu]["median_ms"])
            rec["best"] = {"c": best[0], "T": best[1]}
            rec["baseline_over_best"] = round(rec["baseline"]["median_ms"] / rec["c=%d,T=%d" % best]["median_ms"], 2)
            rec["derived_ratio_at_best"] = round(BASELINE_PRODUCTS / many_products(best[0], min(best[1], lmax)), 2)
        rec["baseline_over_default"] = round(rec["baseline"]["median_ms"] / rec["default"]["median_ms"], 2)
        settings(0, 0, 0)
        emit(rec)

    sweep = [(c, u) for c in cs for u in units]
    for m, ln in shapes:
        run_shape("len=%d" % ln, lambda mm, ln=ln: np.full(mm, ln, np.int64), m, [(c, u) for c, u in sweep if u <= ln or u == 1])
    if args.ragged:
        run_shape("ragged 1..64", lambda mm: (np.arange(mm, dtype=np.int64) % 64) + 1, args.ragged, sweep)
    if args.long:
        run_shape("len=2048", lambda mm: np.full(mm, 2048, np.int64), args.long,
                  [(4, 32)], {"alone": (0, 0, 1024), "packed": (0, 0, 4096)}, reps=args.long_reps)

    if args.kzg:
        m = args.kzg
        ln = 16
        n = 2 * m * ln
        g2 = to_dev(np.tile(synth.g2_one_image(), (2, 1)))
        s2 = to_dev(synth.fr_images_raw(2, 0x6d616e33))
        Q = torch.empty((2, 24), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        ctx.g2_mul_many_dev(g2.data_ptr(), s2.data_ptr(), 2, Q.data_ptr(), sh)
        torch.cuda.synchronize(dev)
        g2h = dctx.g2_prepare_dev(Q.data_ptr(), 2, sh)
        P, K = PTS[:n], SCAL[:n]
        off = np.arange(0, n + 1, ln).astype(np.uintp)
        REP = P.view(2 * m, ln, 12).transpose(0, 1).contiguous()
        Kt = K.view(2 * m, ln, 4).transpose(0, 1).contiguous()
        T = torch.empty((n, 12), dtype=torch.int64, device=dev)
        PAIRS = torch.zeros((2 * m, 12), dtype=torch.int64, device=dev)
        GT = torch.zeros((m, 48), dtype=torch.int64, device=dev)
        qidx = np.tile(np.array([0, 1], np.uint32), m)
        poff = np.arange(0, 2 * m + 1, 2).astype(np.uintp)
        dctx.reserve(2 * m)
        dctx.g1_msm_many_reserve(n, 2 * m)
        torch.cuda.synchronize(dev)

        def products():
            dctx.pairing_batch_prepared_many_dev(PAIRS.data_ptr(), None, g2h, qidx, poff, GT.data_ptr(), sh)

        def with_msm_many():
            dctx.g1_msm_many_dev(P.data_ptr(), K.data_ptr(), off, PAIRS.data_ptr(), 1, sh)
            products()

        def with_baseline():
            dctx.g1_mul_many_dev(REP.data_ptr(), Kt.data_ptr(), n, T.data_ptr(), sh)
            k = ln
            while k > 1:
                h = (k + 1) // 2
                dctx.group_op_many_dev("g1", "add", T.data_ptr(), T.data_ptr() + h * 2 * m * 96, (k - h) * 2 * m,
                                       T.data_ptr(), sh)
                k = h
            dctx.group_op_many_dev("g1", "normalize", T.data_ptr(), None, 2 * m, PAIRS.data_ptr(), sh)
            products()

        forms = {"with_baseline": with_baseline, "with_msm_many": with_msm_many, "pairing_products_alone": products}
        outs = {}
        for name, fn in forms.items():
            timed(fn)
            outs[name] = GT.cpu().numpy().copy()
        if not np.array_equal(outs["with_msm_many"], outs["with_baseline"]):
            print("MISMATCH in the KZG-shaped run", file=sys.stderr)
            sys.exit(1)
        times = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, fn in forms.items():
                times[name].append(timed(fn))
        emit({"kzg": m, "msms": 2 * m, "len": ln, "reps": args.reps, **{name: stats(times[name]) for name in forms}})


if __name__ == "__main__":
    main()
