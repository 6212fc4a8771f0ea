#!/usr/bin/env python3
"""The spatially coupled decoder against the uncoupled one on one shape:
L = M = 512, base matrix (omega = 4, Lambda = 16): R = 19, C = 16, n = 4617
(243 rows per row block, 32 sections per column block), P = 15, binary32.

timing  (recorded, nothing asserted): the device time per iteration of
  sa_sc_amp (events around its launches) at B = 1 and B = 256, T = 32, early
  stop off, beside amp_batch's device-resident form (sa_stage / sa_run, events)
  on the uncoupled operator of the same (L, M, n) and B, and a third leg, the
  coupled kernels at W = [[1]] (one row block, one column block: what the
  one-wave-per-section kernel pair costs without any block structure; no plan
  option forces k_sec on this shape).  One warm-up of every leg, then --rounds
  interleaved rounds; medians and ranges.
payoff: 256 reps (seeds 0..255, drawn as harness._draw_reps draws them) at two
  sigma around the uncoupled decoder's failure point, which a scan of --probe
  reps over --sigmas finds first (the last sigma at which the uncoupled
  decoder's section error rate stays under 1 %, and the next one).  The
  uncoupled decoder gets its iterative power allocation (pa_iterative at the
  code's rate), the coupled one the flat allocation; section error rates of both.
Prints one JSON line and writes it to results/sc.json (or --out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=list(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "sc.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--reps", type=int, default=256)
    ap.add_argument("--probe", type=int, default=32)
    ap.add_argument("--payoff-T", type=int, default=100)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0])
    ap.add_argument("--no-payoff", action="store_true")
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd.harness import draw_reps
    from sparc_ldpc_amd.operators import _cached_operator

    L = M = 512
    omega, Lam, P = 4, 16, 15.0
    W = sp.base_matrix(omega, Lam)
    R, C = W.shape
    n = R * 243
    T = args.T
    rate = L * np.log2(M) / n
    Pl = np.full(L, P / L)
    Ab, Az, ordering = sp.sc_transforms(L, M, n, W, precision=args.precision)
    cop = Ab.op
    fAb, _, _ = sp.sc_transforms(L, M, n, np.ones((1, 1)), precision=args.precision)
    fop = fAb.op
    uop = _cached_operator(L, M, n, ordering, "hadamard", args.precision, None)
    out = dict(workload=f"L={L} M={M} n={n} omega={omega} Lambda={Lam} R={R} C={C} P={P} rate={rate:.4f} bits "
                        f"T={T} {args.precision}, early stop off", timing={})

    sigma_t = 1.2
    for B in args.batches:
        idx, noise = draw_reps(np.arange(B), L, M, n, sigma_t)
        # one y for every leg: the coupled code's channel output
        beta0 = np.zeros((B, L * M))
        for k in range(B):
            beta0[k, np.arange(L) * M + idx[k]] = np.sqrt(n * Pl)
        y = cop.Ab_batch(beta0) + noise
        del beta0
        plan = uop.plan(B)

        def coupled(op=cop):
            op.amp_batch(y, Pl, T, early_stop=False)
            return op.last_amp_ms() / T

        def flat():
            return coupled(fop)

        def uncoupled():
            uop.reserve(B, T)
            uop.stage(y, Pl)
            uop.run(B, T, early_stop=False)
            uop.wait()
            return uop.last_run_ms() / T

        legs = dict(coupled=coupled, uncoupled=uncoupled, coupled_kernels_flat_W=flat)
        for f in legs.values():
            f()  # warm-up
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, f in legs.items():
                ms[k].append(f())
        t = {k: stats(v) for k, v in ms.items()}
        t["uncoupled_plan"] = plan
        t["ratio_coupled_over_uncoupled"] = t["coupled"]["median"] / t["uncoupled"]["median"]
        t["ratio_flat_W_over_uncoupled"] = t["coupled_kernels_flat_W"]["median"] / t["uncoupled"]["median"]
        out["timing"][f"B={B}"] = dict(unit="device ms per iteration", **t)

    if not args.no_payoff:
        Tp = args.payoff_T

        def ser_uncoupled(seeds, sigma):
            Plu = sp.pa_iterative(L, L, sigma, P, rate)  # one block per section, the code's rate
            idx, noise = draw_reps(seeds, L, M, n, sigma)
            B = len(seeds)
            uop.reserve(B, Tp)
            uop.stage_power(B, Plu)
            uop.encode(idx, noise)
            uop.run(B, Tp, early_stop=True)
            dec = uop.decide(B)
            return float((dec != idx).mean())

        def ser_coupled(seeds, sigma):
            errs, its, dec = sp.mc_decode_sc(Ab, Pl, sigma, Tp, seeds, batch=len(seeds))
            idx, _ = draw_reps(seeds, L, M, n, sigma)
            return float((dec != idx).mean()), float(its.mean())

        probe = np.arange(1000, 1000 + args.probe)
        scan = [dict(sigma=s, ser_uncoupled=ser_uncoupled(probe, s)) for s in args.sigmas]
        ok = [i for i, p in enumerate(scan) if p["ser_uncoupled"] < 0.01]
        i0 = max(ok) if ok else 0
        pair = [args.sigmas[i0], args.sigmas[min(i0 + 1, len(args.sigmas) - 1)]]
        seeds = np.arange(args.reps)
        points = []
        for s in pair:
            sc_ser, sc_it = ser_coupled(seeds, s)
            points.append(dict(sigma=s, snr=P / s ** 2, capacity_bits=0.5 * np.log2(1 + P / s ** 2),
                               ser_uncoupled_pa_iterative=ser_uncoupled(seeds, s), ser_coupled_flat=sc_ser,
                               coupled_mean_stop=sc_it))
        out["payoff"] = dict(reps=args.reps, T=Tp, early_stop=True, probe_reps=args.probe, scan=scan, points=points)

    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
