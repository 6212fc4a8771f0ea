#!/usr/bin/env python3
"""What the coupled decoder's tolerance stop and frozen column blocks gain
(recorded, nothing asserted), on bench_sc.py's shape:
L = M = 512, base matrix (omega = 4, Lambda = 16): R = 19, C = 16, n = 4617,
P = 15, flat allocation, binary32, sigma = 1.8, 256 reps with seeds 0..255
(drawn as harness._draw_reps draws them), T = 100 and 300.

Legs: (stop_tol, freeze_tol) = (0, 0), today's decoder, and the grid
--stop-tols x --freeze-tols.  Per leg and T, from one sa_sc_mc_ex call on all
reps (encoder, decode and decisions on the device): the device time (events),
the mean stop index, the codewords that never stopped, the share of
block-iterations in front of the stop that were frozen, and the section error
rate.  The same legs at B = 1 (rep 0), where the grid is under one wave of the
chip.  One warm-up of every leg, then --rounds interleaved rounds; medians and
ranges.  Prints one JSON line and writes it to results/sc_wave.json (or --out)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "sc_wave.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--Ts", type=int, nargs="+", default=[100, 300])
    ap.add_argument("--reps", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=1.8)
    ap.add_argument("--stop-tols", type=float, nargs="+", default=[1e-3, 1e-2])
    ap.add_argument("--freeze-tols", type=float, nargs="+", default=[0.0, 1e-2, 5e-2])
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd.harness import draw_reps

    L = M = 512
    omega, Lam, P = 4, 16, 15.0
    W = sp.base_matrix(omega, Lam)
    R, C = W.shape
    n = R * 243
    Pl = np.full(L, P / L)
    Ab, _, _ = sp.sc_transforms(L, M, n, W, precision=args.precision)
    op = Ab.op
    idx, noise = draw_reps(np.arange(args.reps), L, M, n, args.sigma)
    legs = [(0.0, 0.0)] + [(s, f) for s in args.stop_tols for f in args.freeze_tols]
    out = dict(workload=f"L={L} M={M} n={n} omega={omega} Lambda={Lam} R={R} C={C} P={P} sigma={args.sigma} "
                        f"{args.precision}, flat allocation, early stop on, seeds 0..{args.reps - 1}",
               unit="device ms of one sa_sc_mc_ex call (encoder, decode, decisions)", rounds=args.rounds, runs=[])

    for B in (args.reps, 1):
        ib, nb = idx[:B], noise[:B]
        for T in args.Ts:
            def leg(st, ft):
                dec, its, errs, ms, live = op.mc(ib, nb, Pl, T, stop_tol=st, freeze_tol=ft, return_live=True)
                return ms, dec, its, live

            for st, ft in legs:
                leg(st, ft)  # warm-up
            ms = {k: [] for k in legs}
            last = {}
            for _ in range(args.rounds):
                for k in legs:
                    r = leg(*k)
                    ms[k].append(r[0])
                    last[k] = r[1:]
            base = statistics.median(ms[(0.0, 0.0)])
            for k in legs:
                dec, its, live = last[k]
                ran = int(its.astype(np.int64).sum()) * C   # block-iterations in front of the stop
                out["runs"].append(dict(
                    B=B, T=T, stop_tol=k[0], freeze_tol=k[1], ms=stats(ms[k]),
                    speedup_over_zero=base / statistics.median(ms[k]),
                    mean_stop=float(its.mean()), never_stopped=int((its >= T).sum()),
                    frozen_share=float(ran - int(live.sum())) / ran,
                    section_error_rate=float((dec != ib).mean()),
                    codewords_in_error=int((dec != ib).any(axis=1).sum())))

    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
