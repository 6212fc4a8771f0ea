#!/usr/bin/env python3
"""Coupled state evolution on the device, on the coupled decoder's bench shape:
L = M = 512, base matrix (omega = 4, Lambda = 16): R = 19, C = 16, n = 4617,
P = 15, flat allocation (one class per column block: 16 classes), S = 4096 rows.

Three things are timed, in one process (recorded, nothing asserted):
  sa_sc_se  : sc_state_evolution at sigma = 1.8 and 2.0, T = 100 and 200, with
              and without the frozen-block skip, seeded rows; per run the device
              time (ms_out: the draw and the T iterations, HIP events) and the
              wall time of the call.  One warm-up, then --rounds runs of each.
              The draw's share is timed on its own (T = 1).
  sc_search : omega in {2, 3, 4, 6} x Lambda in {8, 16, 32} as one batch
              (--search-samples rows, --search-T iterations).
  numpy     : the statement (tests/sc_se_ref.py) at sigma = 1.8 at
              --numpy-samples rows and --numpy-T iterations, its wall time, and
              that time scaled to S = 4096, T = 100 (the statement's cost is
              linear in both): labelled as scaled, not measured.
Prints one JSON line and writes it to results/sc_se.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "sc_se.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--Ts", type=int, nargs="+", default=[100, 200])
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1.8, 2.0])
    ap.add_argument("--search-samples", type=int, default=1024)
    ap.add_argument("--search-T", type=int, default=200)
    ap.add_argument("--numpy-samples", type=int, default=256)
    ap.add_argument("--numpy-T", type=int, default=6)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp
    import sc_se_ref

    L = M = 512
    omega, Lam, P = 4, 16, 15.0
    W = sp.base_matrix(omega, Lam)
    R, C = W.shape
    n = R * 243
    S = args.samples
    Pl = np.full(L, P / L)
    out = dict(workload=f"L={L} M={M} n={n} omega={omega} Lambda={Lam} R={R} C={C} P={P} flat allocation "
                        f"({C} classes) S={S}, binary64", sa_sc_se=[])
    sp.sc_state_evolution(Pl, M, n, W, args.sigmas[0], 2, samples=S)  # warm-up
    draw = [sp.sc_state_evolution(Pl, M, n, W, args.sigmas[0], 1, samples=S).ms for _ in range(args.rounds)]
    out["draw_plus_one_iteration_device_ms"] = statistics.median(draw)
    for sigma in args.sigmas:
        for T in args.Ts:
            for skip in (True, False):
                runs = []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    r = sp.sc_state_evolution(Pl, M, n, W, sigma, T, samples=S, skip=skip)
                    runs.append(dict(device_ms=r.ms, wall_s=time.perf_counter() - t0))
                dev = statistics.median(x["device_ms"] for x in runs)
                out["sa_sc_se"].append(dict(
                    sigma=sigma, T=T, skip=skip, runs=runs, device_ms_median=dev,
                    wall_s_median=statistics.median(x["wall_s"] for x in runs),
                    device_us_per_iteration_after_the_draw=1e3 * (dev - out["draw_plus_one_iteration_device_ms"]) / max(T - 1, 1),
                    stop=int(r.stop), ser_final=float(r.ser_all[-1]),
                    phi_final_min=float(r.phi[-1].min()), phi_final_max=float(r.phi[-1].max())))
    omegas, Lambdas = [2, 3, 4, 6], [8, 16, 32]
    t0 = time.perf_counter()
    res = sp.sc_search(L, M, n, P, args.sigmas[0], omegas, Lambdas, args.search_T, samples=args.search_samples)
    out["sc_search"] = dict(grid="4 x 3", omega_values=omegas, Lambda_values=Lambdas, sigma=args.sigmas[0],
                            samples=args.search_samples, T=args.search_T, wall_s=time.perf_counter() - t0,
                            device_ms=res.result.ms, best=list(res.best), n=res.n.tolist(), rate=res.rate.tolist(),
                            ser=res.ser.tolist(), stop=res.stop.tolist(), iters=res.iters.tolist())
    if not args.no_numpy:
        sigma, Tn = args.sigmas[0], args.numpy_T
        U = sp.se_draws(np.arange(args.numpy_samples), M)
        t0 = time.perf_counter()
        phi, tau2, x, miss, E, stop = sc_se_ref.sc_se_ref(Pl, sigma, M, n, W, Tn, U)
        wall = time.perf_counter() - t0
        dev = sp.sc_state_evolution(Pl, M, n, W, sigma, Tn, draws=U)
        scale = (S / args.numpy_samples) * (args.Ts[0] / Tn)
        ref_run = next(x for x in out["sa_sc_se"] if x["sigma"] == sigma and x["T"] == args.Ts[0] and x["skip"])
        out["numpy"] = dict(sigma=sigma, samples=args.numpy_samples, T=Tn, wall_s=wall, device_ms_same_problem=dev.ms,
                            max_abs_phi_difference=float(np.max(np.abs(dev.phi - phi))),
                            misses_equal=bool(np.array_equal(dev.miss, miss)), stop_equal=bool(dev.stop == stop),
                            scaled_to_S_T_s=wall * scale,
                            scaled_note=f"wall_s x (S / samples) x ({args.Ts[0]} / T_numpy): scaled, not measured",
                            scaled_over_sa_sc_se_wall=wall * scale / ref_run["wall_s_median"])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
