#!/usr/bin/env python3
"""State evolution on the device against its NumPy statement, on C2's shape:
L = M = 512, n = 4608, P = 4, sigma = 1.1247, T = 64, S = 4096 rows.

Three things are timed, in one process:
  sa_se     : state_evolution for the uniform allocation (one class) and for
              pa_parameterised(a = 1, f = 0.7) (distinct powers plus a flat
              tail), seeded rows; per run the device time (ms_out: the draw
              and the T iterations, HIP events) and the wall time of the call.
              One warm-up, then --rounds runs of each.
  pa_search : a 16 x 8 grid of (a, f) as one batch (--search-samples rows,
              --search-T iterations).
  numpy     : the statement (tests/se_ref.py) for the pa_parameterised
              allocation at --numpy-samples rows and --numpy-T iterations (what
              finishes in about a minute), its wall time, and that time scaled
              to S = 4096, T = 64 (the statement's cost is linear in both):
              labelled as scaled, not measured.
Prints one JSON line and writes it to results/se.json (or --out)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "se.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--search-samples", type=int, default=1024)
    ap.add_argument("--search-T", type=int, default=32)
    ap.add_argument("--numpy-samples", type=int, default=256)
    ap.add_argument("--numpy-T", type=int, default=12)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp
    import se_ref

    L = M = 512
    P, R = 4.0, 1.0
    n = int(L * np.log2(M) / R)
    sigma = float(np.sqrt(P / 10 ** (10 / 20)))
    C = 0.5 * np.log2(1.0 + P / sigma ** 2)
    allocs = {"uniform": P / L * np.ones(L), "pa_parameterised(a=1, f=0.7)": sp.pa_parameterised(L, C, P, 1.0, 0.7)}
    out = dict(workload="L=%d M=%d n=%d P=%.1f sigma=%.4f T=%d S=%d, binary64" % (L, M, n, P, sigma, args.T, args.samples),
               sa_se={})
    for name, Pl in allocs.items():
        sp.state_evolution(Pl, M, n, sigma, args.T, samples=args.samples)  # warm-up
        runs = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            r = sp.state_evolution(Pl, M, n, sigma, args.T, samples=args.samples)
            runs.append(dict(device_ms=r.ms, wall_s=time.perf_counter() - t0))
        out["sa_se"][name] = dict(
            classes=int(len(np.unique(Pl))), runs=runs,
            device_ms_median=statistics.median(x["device_ms"] for x in runs),
            wall_s_median=statistics.median(x["wall_s"] for x in runs),
            tau2_final=float(r.tau2[-1]), x_final=float(r.x[-1]), ser_final=float(r.ser[-1]))
    a_values, f_values = np.linspace(0.2, 1.7, 16), np.linspace(0.3, 1.0, 8, endpoint=False)
    t0 = time.perf_counter()
    res = sp.pa_search(L, M, n, P, sigma, a_values, f_values, args.search_T, samples=args.search_samples)
    out["pa_search"] = dict(grid="16 x 8", a_values=a_values.tolist(), f_values=f_values.tolist(),
                            samples=args.search_samples, T=args.search_T, wall_s=time.perf_counter() - t0,
                            device_ms=res.result.ms, best=list(res.best), x_best=float(res.x.max()),
                            ser_best=float(res.ser.flat[int(np.argmax(res.x))]),
                            x=res.x.tolist(), ser=res.ser.tolist(), iters=res.iters.tolist())
    if not args.no_numpy:
        Pl = allocs["pa_parameterised(a=1, f=0.7)"]
        U = sp.se_draws(np.arange(args.numpy_samples), M)
        t0 = time.perf_counter()
        t2, x, miss, _ = se_ref.se_ref(Pl, sigma, M, n, args.numpy_T, U)
        wall = time.perf_counter() - t0
        dev = sp.state_evolution(Pl, M, n, sigma, args.numpy_T, draws=U)
        scale = (args.samples / args.numpy_samples) * (args.T / args.numpy_T)
        out["numpy"] = dict(allocation="pa_parameterised(a=1, f=0.7)", samples=args.numpy_samples, T=args.numpy_T,
                            wall_s=wall, device_ms_same_problem=dev.ms,
                            max_abs_tau2_difference=float(np.max(np.abs(dev.tau2 - t2[0]))),
                            misses_equal=bool(np.array_equal(dev.miss, miss[0])),
                            scaled_to_S_T_s=wall * scale,
                            scaled_note="wall_s x (S / samples) x (T / T_numpy): scaled, not measured")
        med = out["sa_se"]["pa_parameterised(a=1, f=0.7)"]["wall_s_median"]
        out["numpy"]["scaled_over_sa_se_wall"] = wall * scale / med
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
