#!/usr/bin/env python3
"""Device time of m pairing products of k terms each (n = m * k pairs), three ways, from
HBM-resident inputs, HIP events on the launch stream, after a warm-up of every shape
(which also allocates):
  a  bn_pairing_batch_many_dev, the packed path forced (bn_set_products_min(0))
  b  m sequential bn_pairing_batch_dev calls, one product each.  Above --sample products
     only the first --sample are run and the time is scaled by m / sample: an
     EXTRAPOLATION (the record says "b_extrapolated": true), fair because every call does
     the same work on the same path
  c  bn_pairing_many_dev over the same n pairs: n separate pairings, whose Gt the caller
     would still have to multiply per product
Before a shape is timed, the rows of (a) must equal those of (b) on the products (b) ran,
else the script exits non-zero.  One JSON line per shape with the median / min / max of
each form and terms/s and products/s of the medians; then per k the crossover: the
smallest m from which (a) stays below (b).
--forms picks the forms (a library without the new entry point can still run c: the
baseline of an earlier commit through $BN254MI_LIB).

--prepared F: instead, products of k terms whose first F are fresh and whose others are
drawn from a bn_g2_prepared handle of nq = 3 points (a Groth16 product is k = 4, F = 1), two
ways in the same alternating rounds:
  p  bn_pairing_batch_prepared_many_dev (the fresh terms' G2 points compacted)
  a  bn_pairing_batch_many_dev on the same terms with every G2 point written out
The rows of the two must be equal before a shape is timed, else the script exits non-zero.
One JSON line per shape with both forms and p's time over a's.

--wide: the wide path against the route the call takes without it, for three
kinds of product -- "fresh4" (k = 4, bn_pairing_batch_many_dev), "groth16" (k = 4, one fresh
term and three prepared) and "prepared2" (k = 2, both prepared; both through
bn_pairing_batch_prepared_many_dev) -- over --wide-ms products.  Per shape one warm-up of both
routes, the rows of the two compared (a difference exits non-zero), then --reps alternating
rounds: "wide" with bn_set_products_wide_max above the call, "base" with 0, every other
setting at its default.  One JSON line per shape with median / min / max of both, the routes
each planned (bn_get_products_routes) and wide_wins = wide's median below base's minimum;
then per kind the crossover -- the largest term count up to which wide_wins held at every
shape of the sweep -- and the smallest of the three, the default the sweep supports."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "paritytech-bn_amd"))
sys.path.insert(0, ROOT)

NMAX = 1 << 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--ms", default=",".join(str(1 << e) for e in range(0, 17)))
    ap.add_argument("--forms", default="a,b,c")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sample", type=int, default=32, help="products form b runs at most")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--prepared", type=int, default=None, metavar="F",
                    help="time the prepared-terms call: the first F terms of each product are fresh")
    ap.add_argument("--wide", action="store_true", help="time the wide path against the route without it")
    ap.add_argument("--wide-ms", default="1,2,8,64,256,1024,2048,4096,8192")
    ap.add_argument("--wide-kinds", default="fresh4,groth16,prepared2")
    args = ap.parse_args()
    import torch

    from substrate_bn import Context, synth

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    forms = args.forms.split(",")
    ks = [int(v) for v in args.ks.split(",")]
    ms = [int(v) for v in args.ms.split(",")]
    if args.wide:
        ks, ms = [4], [int(v) for v in args.wide_ms.split(",")]
    shapes = [(k, m) for k in ks for m in ms if m * k <= NMAX]
    nmax = max(m * k for k, m in shapes)
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    if "a" in forms and not args.wide:
        ctx.set_products_min(0)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    # P[i] = s[i] * G1, Q[i] = t[i] * G2 on the device (Jacobian images)
    s, t = up(synth.fr_images_raw(nmax, 0x70726f31)), up(synth.fr_images_raw(nmax, 0x70726f32))
    g1 = up(np.tile(synth.g1_one_image(), (nmax, 1)))
    g2 = up(np.tile(synth.g2_one_image(), (nmax, 1)))
    P = torch.empty((nmax, 12), dtype=torch.int64, device=dev)
    Q = torch.empty((nmax, 24), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_many_dev(g1.data_ptr(), s.data_ptr(), nmax, P.data_ptr(), sh)
    ctx.g2_mul_many_dev(g2.data_ptr(), t.data_ptr(), nmax, Q.data_ptr(), sh)
    torch.cuda.synchronize(dev)
    del s, t, g1, g2
    ctx.reserve(min(nmax, NMAX))
    out_a = torch.zeros((max(ms), 48), dtype=torch.int64, device=dev)
    out_b = torch.zeros((args.sample, 48), dtype=torch.int64, device=dev)
    out_c = torch.zeros((nmax, 48), dtype=torch.int64, device=dev)
    g1_bytes, g2_bytes, gt_bytes = 96, 192, 384

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def run(form, k, m):
        """-> milliseconds for the whole shape (form b: scaled up from its sample)"""
        n = m * k
        if form == "a":
            off = np.arange(m + 1, dtype=np.uintp) * k
            return timed(lambda: ctx.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), off, out_a.data_ptr(), sh))
        if form == "b":
            ran = min(m, args.sample)

            def calls():
                for j in range(ran):
                    ctx.pairing_batch_dev(P.data_ptr() + j * k * g1_bytes, Q.data_ptr() + j * k * g2_bytes, k,
                                          out_b.data_ptr() + j * gt_bytes, None, sh)
            return timed(calls) * m / ran
        return timed(lambda: ctx.pairing_many_dev(P.data_ptr(), Q.data_ptr(), n, out_c.data_ptr(), sh))

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    if args.wide:
        wide_sweep(args, ctx, torch, dev, sh, ms, P, Q, timed, stats, emit)
        return
    if args.prepared is not None:
        prepared_sweep(args, ctx, torch, dev, sh, shapes, P, Q, timed, stats, emit)
        return

    cross = {k: None for k in ks}
    for k, m in shapes:
        for f in forms:  # warm-up
            run(f, k, m)
        ctx.dev_status()
        if "a" in forms and "b" in forms:
            ran = min(m, args.sample)
            if not np.array_equal(out_a[:ran].cpu().numpy(), out_b[:ran].cpu().numpy()):
                print("MISMATCH at k=%d m=%d: the packed rows differ from bn_pairing_batch_dev's" % (k, m), file=sys.stderr)
                sys.exit(1)
        times = {f: [] for f in forms}
        for _ in range(args.reps):
            for f in forms:  # alternating
                times[f].append(run(f, k, m))
        rec = {"k": k, "m": m, "n": m * k, "reps": args.reps}
        for f in forms:
            st = stats(times[f])
            st["terms_per_s"] = round(m * k / (st["median_ms"] * 1e-3))
            st["products_per_s"] = round(m / (st["median_ms"] * 1e-3))
            rec[f] = st
        if "b" in forms:
            rec["b_extrapolated"] = m > args.sample
        if "a" in forms and "b" in forms:
            if rec["a"]["median_ms"] < rec["b"]["median_ms"]:
                if cross[k] is None:
                    cross[k] = m
            else:
                cross[k] = None
        emit(rec)
    ctx.dev_status()
    if "a" in forms and "b" in forms:
        emit({"crossover_m": {str(k): cross[k] for k in ks},
              "note": "smallest m of the sweep from which the packed path stays below m single-product calls"})


def prepared_sweep(args, ctx, torch, dev, sh, shapes, P, Q, timed, stats, emit):
    """The --prepared F sweep over `shapes` = [(k, m)]: the handle's points are Q[0 .. 2], a
    product's prepared terms take them in turn, its fresh terms take Q from row 3 on."""
    F, nq = args.prepared, 3
    handle = ctx.g2_prepare_dev(Q.data_ptr(), nq, sh)
    out_p = torch.zeros((max(m for _, m in shapes), 48), dtype=torch.int64, device=dev)
    out_a = torch.zeros_like(out_p)
    for k, m in shapes:
        f = min(F, k)
        n = m * k
        off = np.arange(m + 1, dtype=np.uintp) * k
        t = np.arange(n) % k                                  # position inside the product
        fresh = t < f
        qidx = np.where(fresh, 0xFFFFFFFF, (t - f) % nq).astype(np.uint32)
        nf = int(fresh.sum())
        with torch.cuda.stream(torch.cuda.ExternalStream(sh)):
            base = nq if nq + nf <= Q.shape[0] else 0
            Qf = Q[base:base + nf].contiguous() if nf else Q[:1]  # the compacted fresh points
            Qfull = torch.empty((n, 24), dtype=torch.int64, device=dev)
            mask = torch.from_numpy(fresh).to(dev)
            if nf:
                Qfull[mask] = Qf
            if nf < n:
                Qfull[~mask] = Q[torch.from_numpy(qidx[~fresh].astype(np.int64)).to(dev)]
        torch.cuda.synchronize(dev)

        def run(form):
            if form == "p":
                return timed(lambda: ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qf.data_ptr(), handle, qidx,
                                                                         off, out_p.data_ptr(), sh))
            return timed(lambda: ctx.pairing_batch_many_dev(P.data_ptr(), Qfull.data_ptr(), off, out_a.data_ptr(), sh))

        for form in ("p", "a"):  # warm-up
            run(form)
        ctx.dev_status()
        if not np.array_equal(out_p[:m].cpu().numpy(), out_a[:m].cpu().numpy()):
            print("MISMATCH at k=%d m=%d F=%d: the prepared call's rows differ from bn_pairing_batch_many_dev's"
                  % (k, m, f), file=sys.stderr)
            sys.exit(1)
        times = {"p": [], "a": []}
        for _ in range(args.reps):
            for form in ("p", "a"):  # alternating
                times[form].append(run(form))
        rec = {"k": k, "m": m, "n": n, "fresh": f, "nq": nq, "reps": args.reps}
        for form in ("p", "a"):
            st = stats(times[form])
            st["products_per_s"] = round(m / (st["median_ms"] * 1e-3))
            rec[form] = st
        rec["p_over_a"] = round(rec["p"]["median_ms"] / rec["a"]["median_ms"], 4)
        emit(rec)
    ctx.dev_status()
    ctx.g2_prepared_destroy(handle)


def wide_sweep(args, ctx, torch, dev, sh, ms, P, Q, timed, stats, emit):
    """The --wide sweep: the handle's points are Q[0 .. 2]; a product's fresh terms take Q from
    row 3 on (compacted for the prepared call)."""
    nq, big = 3, 1 << 30
    kinds = {"fresh4": (4, 4), "groth16": (4, 1), "prepared2": (2, 0)}  # k, fresh terms per product
    handle = ctx.g2_prepare_dev(Q.data_ptr(), nq, sh)
    out_w = torch.zeros((max(ms), 48), dtype=torch.int64, device=dev)
    out_b = torch.zeros_like(out_w)
    cross = {}
    for kind in args.wide_kinds.split(","):
        k, f = kinds[kind]
        wins = True
        cross[kind] = 0
        for m in ms:
            n = m * k
            off = np.arange(m + 1, dtype=np.uintp) * k
            qidx = np.where(np.arange(n) % k < f, 0xFFFFFFFF, (np.arange(n) % k - f) % nq).astype(np.uint32)
            Qf = Q[nq:]                                        # contiguous rows: the compacted fresh points

            def call(out):
                if kind == "fresh4":
                    ctx.pairing_batch_many_dev(P.data_ptr(), Q.data_ptr(), off, out.data_ptr(), sh)
                else:
                    ctx.pairing_batch_prepared_many_dev(P.data_ptr(), Qf.data_ptr(), handle, qidx, off,
                                                        out.data_ptr(), sh)

            def run(route):
                ctx.set_products_wide_max(big if route == "wide" else 0)
                ctx.products_routes()
                ms_ = timed(lambda: call(out_w if route == "wide" else out_b))
                return ms_, ctx.products_routes()

            routes = {r: run(r)[1] for r in ("wide", "base")}  # warm-up (allocates)
            ctx.dev_status()
            if not np.array_equal(out_w[:m].cpu().numpy(), out_b[:m].cpu().numpy()):
                print("MISMATCH at %s m=%d: the wide rows differ from the base route's" % (kind, m), file=sys.stderr)
                sys.exit(1)
            times = {"wide": [], "base": []}
            for _ in range(args.reps):
                for r in ("wide", "base"):  # alternating
                    times[r].append(run(r)[0])
            rec = {"kind": kind, "k": k, "fresh": f, "m": m, "n": n, "reps": args.reps,
                   "wide": stats(times["wide"]), "base": stats(times["base"]),
                   "routes_wide": routes["wide"], "routes_base": routes["base"]}
            rec["wide_wins"] = rec["wide"]["median_ms"] < rec["base"]["min_ms"]
            same_route = routes["wide"] == routes["base"]      # (one fresh product: alone either way)
            if not same_route:
                wins = wins and rec["wide_wins"]
                if wins:
                    cross[kind] = n
            emit(rec)
    ctx.dev_status()
    ctx.set_products_wide_max(0)
    ctx.g2_prepared_destroy(handle)
    emit({"crossover_terms": cross, "supported_default": min(cross.values()),
          "note": "per kind the largest term count up to which the wide route's median stayed below the base "
                  "route's minimum at every shape of the sweep; the default is the smallest of them"})


if __name__ == "__main__":
    main()
