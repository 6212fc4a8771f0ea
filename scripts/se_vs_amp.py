#!/usr/bin/env python3
"""State evolution against the decoder itself, on C2 (L = M = 512, n = 4608,
P = 4, uniform allocation): how far SE's tau_t^2 and section error rate are
from what 256 decoded codewords show, at two sigma.

SE is exact as L grows; at a finite L the decoder's empirical values sit off
it by a gap nobody had measured.  No test asserts it: this script records it.

Per sigma the decoder runs the same 256 codewords (seeded reps, early stop
off) with T = t for t = 1..8.  After t iterations
  tau2_amp[t] = mean over codewords of |z_t|^2 / n   (sa_fetch_z), against SE's tau2[t];
  ser_amp[t]  = wrong sections / (256 L)             (sa_decide),  against SE's ser[t - 1]
(the estimate of iteration t is formed at the noise level tau_{t-1}).  SE runs
on --samples rows.  Prints one JSON line and writes results/se_vs_amp.json (or
--out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "se_vs_amp.json"))
    ap.add_argument("--codewords", type=int, default=256)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1.1247, 1.0])
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp

    L = M = 512
    P = 4.0
    n = int(L * np.log2(M))
    B, K = args.codewords, args.iterations
    Pl = P / L * np.ones(L)
    op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=args.precision)
    op.reserve(B, K)
    op.stage_power(B, Pl)
    out = dict(workload="L=%d M=%d n=%d P=%.1f uniform, %d codewords, %s; SE on %d rows" % (
        L, M, n, P, B, args.precision, args.samples), points=[])
    for sigma in args.sigmas:
        se = sp.state_evolution(Pl, M, n, sigma, K, samples=args.samples)
        idx, noise = sp.draw_reps(list(range(B)), L, M, n, sigma)
        tau2_amp, tau2_sd, ser_amp = [], [], []
        for t in range(1, K + 1):
            op.encode(idx, noise)
            op.run(B, t, early_stop=False)
            z = op.fetch_z(B)
            t2 = (z ** 2).sum(axis=1) / n
            tau2_amp.append(float(t2.mean()))
            tau2_sd.append(float(t2.std()))
            ser_amp.append(float((op.decide(B) != idx).mean()))
        y2 = float((op.fetch_y(B) ** 2).sum(axis=1).mean() / n)
        out["points"].append(dict(
            sigma=sigma, tau2_se=se.tau2.tolist(), ser_se=se.ser.tolist(), tau2_amp_0=y2, tau2_amp=tau2_amp,
            tau2_amp_std_over_codewords=tau2_sd, ser_amp=ser_amp,
            tau2_relative_gap=[(a - s) / s for a, s in zip(tau2_amp, se.tau2[1:])],
            ser_gap=[a - s for a, s in zip(ser_amp, se.ser)]))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
