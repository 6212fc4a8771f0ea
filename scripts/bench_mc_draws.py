#!/usr/bin/env python3
"""The configs[3] sweep end to end, host draws against device draws: L=768
M=512 at the sweep's rate (n=8294), P=1.8, T=64, 10 sigma points x 1000 reps
as ONE stream through 256 slots, fp32, on an operator that already exists.

Each run is timed on the host clock from the seed list to the per-rep results
(every path ends in a device synchronise inside the library):
  host   : draw_reps (native draws on the host cores) -> mc_stream (stage: the
           fp64 noise and the indices go up; then the stream)
  device : mc_stream_seeds (the seeds and sigmas go up; sa_mc_draw; the stream)
One warm-up of each path, then the two alternate for --rounds rounds (>= 5) in
one process.  Per run the split: draw, stage, stream device ms, total.  The bar
(DESIGN section 8): every device-draw run below every host-draw run.  Prints
one JSON line and writes it to results/mc_draws.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "mc_draws.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1000, help="reps per sigma point")
    ap.add_argument("--points", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    assert args.rounds >= 1
    import sparc_ldpc_amd as sp
    L, M, P, T = 768, 512, 1.8, 64
    logm = np.log2(M)
    R = 5 / 6
    n = int(L * logm / R)
    Pl = P / L * np.ones(L)
    sigmas = np.linspace(0.8, 0.4, 10)[:args.points]
    seeds = [list(range(i * 100000, i * 100000 + args.reps)) for i in range(len(sigmas))]
    all_seeds = [s for pt in seeds for s in pt]
    all_sigma = np.repeat(sigmas, args.reps)
    nrep = len(all_seeds)
    op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision="fp32")
    assert op.mc_supported(args.batch)
    op.reserve(args.batch, T)
    idx = np.empty((nrep, L), dtype=np.int32)
    noise = np.empty((nrep, n))

    def host():
        t0 = time.perf_counter()
        for i, sg in enumerate(sigmas):
            sl = slice(i * args.reps, (i + 1) * args.reps)
            sp.draw_reps(seeds[i], L, M, n, sg, idx=idx[sl], noise=noise[sl])
        t1 = time.perf_counter()
        tm = {}
        be, it, ms = sp.mc_stream(op, Pl, T, idx, noise, batch=args.batch, timings=tm)
        t2 = time.perf_counter()
        return be, it, dict(total_s=t2 - t0, draw_s=t1 - t0, stage_s=tm["stage_s"], stream_device_ms=ms,
                            run_s=tm["run_s"])

    def device():
        t0 = time.perf_counter()
        tm = {}
        be, it, ms = sp.mc_stream_seeds(op, Pl, T, all_seeds, all_sigma, batch=args.batch, timings=tm)
        t1 = time.perf_counter()
        return be, it, dict(total_s=t1 - t0, draw_s=tm["draw_ms"] / 1e3, stage_s=tm["stage_s"], stream_device_ms=ms,
                            run_s=tm["run_s"])

    be_h, it_h, _ = host()
    be_d, it_d, _ = device()
    runs_h, runs_d = [], []
    for _ in range(args.rounds):
        runs_h.append(host()[2])
        runs_d.append(device()[2])
    th = [r["total_s"] for r in runs_h]
    td = [r["total_s"] for r in runs_d]
    bits = nrep * L * logm
    out = dict(
        workload="L=%d M=%d n=%d P=%.1f T=%d, %d sigma x %d reps, %d slots, fp32" % (
            L, M, n, P, T, len(sigmas), args.reps, args.batch),
        host_draws=dict(runs=runs_h, median_s=statistics.median(th), reps_per_s=nrep / statistics.median(th)),
        device_draws=dict(runs=runs_d, median_s=statistics.median(td), reps_per_s=nrep / statistics.median(td)),
        split_note="total_s: host clock from the seed list to the per-rep results; draw_s: the host draws' wall time / "
                   "the device draw's event time (inside stage_s); stage_s: sa_mc_stage (upload) / sa_mc_draw "
                   "(seed upload + draw); stream_device_ms: events around the stream; run_s: sa_mc_run's wall time",
        speedup=statistics.median(th) / statistics.median(td),
        bar_every_device_run_below_every_host_run=bool(max(td) < min(th)),
        # the two paths decode noise that differs in a last bit of a few values in a thousand
        reps_with_a_different_result=int(((be_h != be_d) | (it_h != it_d)).sum()),
        ber_host=float(be_h.sum() / bits), ber_device=float(be_d.sum() / bits),
    )
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
