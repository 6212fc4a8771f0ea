#!/usr/bin/env python3
"""Coupled state evolution against the coupled decoder itself, on the decoder's
bench shape (L = M = 512, (omega, Lambda) = (4, 16): R = 19, C = 16, n = 4617,
P = 15, flat allocation), at sigma = 1.8 and 2.0: the two rows of the payoff
table of DESIGN.md section 13.

SE is exact as the blocks grow; at 32 sections a column block the decoder's
empirical values sit off it by a finite-size gap.  No test asserts it: this
script records it.

Per sigma, --codewords seeded reps (seeds 0 .., drawn as harness.draw_reps
draws them) are decoded twice: with the early stop off for the phi trace
(amp_sc_batch, T iterations, in batches of --batch), and through mc_decode_sc
with the early stop on for the stop indices and the decisions.  SE runs on
--samples rows for --se-T iterations.  Recorded:
  phi_relative_gap[t] = max_r |mean over codewords of phi_r^t - SE's phi_r^t| / SE's phi_r^t, t < T;
  the predicted stop index against the decoder's mean (and range);
  the predicted section error rate after T and after --se-T iterations
  against the decoder's after T;
  whether SE's wave completes (every column block's predicted section error
  rate under 5 %) and the first iteration at which it does, which at
  sigma = 2.0 answers whether a larger T would help the decoder; and the
  decoder's section error rate and stop indices at that larger T (--long-T,
  early stop on), which says whether it did.
Prints one JSON line and writes results/sc_se_vs_amp.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "sc_se_vs_amp.json"))
    ap.add_argument("--codewords", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--se-T", type=int, default=400)
    ap.add_argument("--long-T", type=int, default=300)
    ap.add_argument("--sigmas", type=float, nargs="+", default=[1.8, 2.0])
    ap.add_argument("--precision", default="fp32")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd.harness import draw_reps

    L = M = 512
    omega, Lam, P = 4, 16, 15.0
    W = sp.base_matrix(omega, Lam)
    R, C = W.shape
    n = R * 243
    T, B = args.T, args.codewords
    Pl = np.full(L, P / L)
    Ab, Az, _ = sp.sc_transforms(L, M, n, W, precision=args.precision)
    op = Ab.op
    seeds = np.arange(B)
    out = dict(workload=f"L={L} M={M} n={n} omega={omega} Lambda={Lam} R={R} C={C} P={P} flat allocation, {B} codewords, "
                        f"{args.precision}, T={T}; SE on {args.samples} rows, T={args.se_T}", points=[])
    for sigma in args.sigmas:
        se = op.state_evolution(Pl, sigma, args.se_T, samples=args.samples)
        done = np.flatnonzero((se.ser < 0.05).all(axis=1))
        phi_sum = np.zeros((T, R))
        for i0 in range(0, B, args.batch):
            idx, noise = draw_reps(seeds[i0:i0 + args.batch], L, M, n, sigma)
            beta0 = np.zeros((len(idx), L * M))
            for k in range(len(idx)):
                beta0[k, np.arange(L) * M + idx[k]] = np.sqrt(n * Pl)
            y = op.Ab_batch(beta0) + noise
            del beta0
            _, _, phi = op.amp_batch(y, Pl, T, early_stop=False)
            phi_sum += phi.sum(axis=0)
        phi_amp = phi_sum / B
        errs, its, dec = sp.mc_decode_sc(Ab, Pl, sigma, T, seeds, batch=args.batch)
        idx, _ = draw_reps(seeds, L, M, n, sigma)
        wrong = dec != idx
        _, its_long, dec_long = sp.mc_decode_sc(Ab, Pl, sigma, args.long_T, seeds, batch=args.batch)
        gap = np.abs(phi_amp - se.phi[:T]) / se.phi[:T]
        out["points"].append(dict(
            sigma=sigma, snr=P / sigma ** 2,
            phi_relative_gap=gap.max(axis=1).tolist(), phi_relative_gap_row_block=gap.argmax(axis=1).tolist(),
            phi_se_min=se.phi.min(axis=1).tolist(), phi_se_max=se.phi.max(axis=1).tolist(),
            phi_amp_min=phi_amp.min(axis=1).tolist(), phi_amp_max=phi_amp.max(axis=1).tolist(),
            stop_se=int(se.stop), stop_amp_mean=float(its.mean()), stop_amp_min=int(its.min()), stop_amp_max=int(its.max()),
            ser_se=se.ser_all.tolist(), ser_se_after_T=float(se.ser_all[min(T, args.se_T) - 1]),
            ser_se_final=float(se.ser_all[-1]), ser_amp_after_T=float(wrong.mean()),
            ser_amp_per_column_block=wrong.reshape(B, C, L // C).mean(axis=(0, 2)).tolist(),
            ser_se_per_column_block_after_T=se.ser[min(T, args.se_T) - 1].tolist(),
            ser_se_column_block_max=se.ser.max(axis=1).tolist(),
            se_wave_completes=bool(done.size), se_wave_complete_at=int(done[0]) + 1 if done.size else None,
            se_wave_completes_within_T=bool(done.size and done[0] + 1 <= T),
            long_T=args.long_T, ser_amp_after_long_T=float((dec_long != idx).mean()),
            stop_amp_mean_long_T=float(its_long.mean()), stop_amp_max_long_T=int(its_long.max()),
            codewords_stopped_before_long_T=int((its_long < args.long_T).sum())))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
