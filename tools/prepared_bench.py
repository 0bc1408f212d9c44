#!/usr/bin/env python3
"""Device time of n pairings against prepared G2 points, from HBM-resident inputs, HIP events
on the launch stream, after a warm-up of every shape (which also allocates), in interleaved
rounds:
  a  bn_pairing_prepared_many_dev, a handle of nq = 1 point, qidx NULL
  b  bn_pairing_prepared_many_dev, nq = 4, random indices
  c  bn_pairing_prepared_many_dev, nq = 4096, random indices (a 77 MB table: past L2)
  d  bn_pairing_many_dev over the pairs of form c: the baseline, code the prepared calls do
     not touch (at n <= 8192 it takes the latency path, above it k_pairing_full)
Before a shape is timed, the rows of each prepared form must equal bn_pairing_many_dev's on
the same pairs (the G2 points gathered by the form's indices), else the script exits
non-zero.  One JSON line per shape with the median / min / max of each form and pairings/s of
the medians.  --forms picks the forms; --out also appends the lines to a file."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "paritytech-bn_amd"))
sys.path.insert(0, ROOT)

NQ = {"a": 1, "b": 4, "c": 4096}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default=",".join(str(1 << e) for e in (10, 12, 14, 16, 18)))
    ap.add_argument("--forms", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=7)
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

    forms = args.forms.split(",")
    ns = [int(v) for v in args.ns.split(",")]
    nmax = max(ns)
    nqmax = max(NQ.values())
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    stream = torch.cuda.Stream(dev)
    sh = stream.cuda_stream

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)

    # P[i] = s[i] * G1, Q[j] = t[j] * G2 on the device (Jacobian images)
    s, t = up(synth.fr_images_raw(nmax, 0x70726531)), up(synth.fr_images_raw(nqmax, 0x70726532))
    g1 = up(np.tile(synth.g1_one_image(), (nmax, 1)))
    g2 = up(np.tile(synth.g2_one_image(), (nqmax, 1)))
    P = torch.empty((nmax, 12), dtype=torch.int64, device=dev)
    Q = torch.empty((nqmax, 24), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ctx.g1_mul_many_dev(g1.data_ptr(), s.data_ptr(), nmax, P.data_ptr(), sh)
    ctx.g2_mul_many_dev(g2.data_ptr(), t.data_ptr(), nqmax, Q.data_ptr(), sh)
    torch.cuda.synchronize(dev)
    del s, t, g1, g2
    ctx.reserve(min(nmax, 1 << 18))
    handles = {f: ctx.g2_prepare_dev(Q.data_ptr(), NQ[f], sh) for f in "abc"}
    torch.cuda.synchronize(dev)
    rng = np.random.default_rng(0x70726533)
    idx_h = {"a": np.zeros(nmax, np.int64), "b": rng.integers(0, NQ["b"], nmax), "c": rng.integers(0, NQ["c"], nmax)}
    idx32 = {f: torch.from_numpy(idx_h[f].astype(np.uint32).view(np.int32)).to(dev) for f in "bc"}
    # the pairs of each prepared form as bn_pairing_many_dev takes them
    Qg = {f: Q[torch.from_numpy(idx_h[f]).to(dev)].contiguous() for f in "abc"}
    out = {f: torch.zeros((nmax, 48), dtype=torch.int64, device=dev) for f in "abcd"}
    ref = torch.zeros((nmax, 48), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    def run(form, n):
        if form == "d":
            return timed(lambda: ctx.pairing_many_dev(P.data_ptr(), Qg["c"].data_ptr(), n, out["d"].data_ptr(), sh))
        qi = None if form == "a" else idx32[form].data_ptr()
        return timed(lambda: ctx.pairing_prepared_many_dev(P.data_ptr(), handles[form], qi, n, out[form].data_ptr(), sh))

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}

    for n in ns:
        for f in forms:  # warm-up
            run(f, n)
        ctx.dev_status()
        for f in forms:
            if f == "d":
                continue
            ctx.pairing_many_dev(P.data_ptr(), Qg[f].data_ptr(), n, ref.data_ptr(), sh)
            ctx.dev_status(sh)
            torch.cuda.synchronize(dev)
            if not torch.equal(out[f][:n], ref[:n]):
                print("MISMATCH at n=%d form %s: the prepared rows differ from bn_pairing_many_dev's" % (n, f),
                      file=sys.stderr)
                sys.exit(1)
        times = {f: [] for f in forms}
        for _ in range(args.reps):
            for f in forms:  # alternating
                times[f].append(run(f, n))
        rec = {"n": n, "reps": args.reps, "checked_against_pairing_many_dev": [f for f in forms if f != "d"]}
        for f in forms:
            st = stats(times[f])
            st["pairings_per_s"] = round(n / (st["median_ms"] * 1e-3))
            if f != "d":
                st["nq"] = NQ[f]
            rec[f] = st
        if "a" in forms and "d" in forms:
            rec["a_over_d"] = round(rec["a"]["median_ms"] / rec["d"]["median_ms"], 4)
        emit(rec)
    ctx.dev_status()
    for h in handles.values():
        ctx.g2_prepared_destroy(h)


if __name__ == "__main__":
    main()
