#!/usr/bin/env python3
"""mc_joint end to end on BASELINE configs[4], host draws against device draws:
L=M=512 P=4 r_sparc=1 (n=4608), T=64, 802.16 rate-5/6 z=192 over all 512
sections, mode soft with 2 rounds, 256 seeds a round at Eb/N0 = 6.89 dB
(scripts/bench_joint.py's point), on decoders that already exist.

Each round is timed on the host clock from the seed list to the per-rep error
counts (every path ends in a device synchronise inside the libraries):
  host   : mc_joint(draws="host"): RandomState per rep, NumPy LDPC encoder and
           bit packing on the host, the indices and the fp64 noise go up
  device : mc_joint(draws="device"): the seeds go up (lb_joint_draw,
           sa_encode_bits), the indices come back
One warm-up round of each leg, then the legs alternate for --rounds rounds
(>= 5) in one process, every round on fresh seeds (the same for both legs).  Two
settings: the default decoder (binary64 AMP, reference LLR) and
precision="fp32", llr="two_sided".  The bar (DESIGN section 8's convention): the
device leg counts as faster only if every device-draw round is below every
host-draw round.  Per leg the per-column BER over the rounds' reps (the same
seeds; the noise differs within the device library's log) and the reps whose
counts differ between the legs.  Prints one JSON line and writes it to
results/joint_draws.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, M, P, T, Z, N_SPARC = 512, 512, 4.0, 64, 192, 4608
EBNO = 6.888888888888889


def columns(r):
    """The per-rep counts of one mc_joint result, column by column (amp rounds, then ldpc rounds)."""
    return np.concatenate([r["amp"], r["ldpc"]], axis=1)


def setting(name, jd, Pl, sigma, rounds, batch, soft_iter):
    from sparc_ldpc_amd.joint import mc_joint
    total_bits = jd.total_bits

    def leg(draws, seeds):
        t0 = time.perf_counter()
        r = mc_joint(jd, Pl, sigma, seeds, "soft", soft_iter, batch, draws=draws)
        return time.perf_counter() - t0, r

    warm = list(range(9000, 9000 + batch))
    leg("host", warm)
    leg("device", warm)
    th, td, draw_ms = [], [], []
    ch, cd = [], []
    for k in range(rounds):
        seeds = list(range(20000 + k * batch, 20000 + (k + 1) * batch))
        s, r = leg("host", seeds)
        th.append(s)
        ch.append(columns(r))
        s, r = leg("device", seeds)
        td.append(s)
        cd.append(columns(r))
        # the pipeline's slices draw beside each other: the slowest slice's event time
        parts = jd._pipeline.parts if jd._pipeline is not None else [jd]
        draw_ms.append(max(p.last_draw_ms for p in parts))
    ch, cd = np.concatenate(ch), np.concatenate(cd)
    names = [f"amp_{i}" for i in range(soft_iter + 1)] + [f"ldpc_{i}" for i in range(soft_iter)]
    nrep = len(ch)
    return dict(
        setting=name,
        host_draws=dict(rounds_s=th, median_s=statistics.median(th), min_s=min(th), max_s=max(th)),
        device_draws=dict(rounds_s=td, median_s=statistics.median(td), min_s=min(td), max_s=max(td),
                          draw_ms_out=draw_ms),
        speedup_of_medians=statistics.median(th) / statistics.median(td),
        bar_every_device_round_below_every_host_round=bool(max(td) < min(th)),
        reps=nrep,
        ber_columns=names,
        ber_host=(ch.sum(axis=0) / (nrep * total_bits)).tolist(),
        ber_device=(cd.sum(axis=0) / (nrep * total_bits)).tolist(),
        reps_with_a_different_count=int((ch != cd).any(axis=1).sum()),
    )


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "joint_draws.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="seeds a round")
    ap.add_argument("--soft-iter", type=int, default=2)
    args = ap.parse_args()
    assert args.rounds >= 1
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import joint
    from sparc_ldpc_amd.harness import ebno_to_sigma
    lp = sp.LDPCParams("802.16", "5/6", Z)
    sigma = ebno_to_sigma(EBNO, P, 5 / 6)
    Pl = P / L * np.ones(L)
    out = dict(
        workload="BASELINE configs[4]: L=%d M=%d n=%d P=%.0f T=%d + 802.16 5/6 z=%d, mode soft x%d, %d seeds a round, "
                 "Eb/N0 %.2f dB (sigma %.6f)" % (L, M, N_SPARC, P, T, Z, args.soft_iter, args.batch, EBNO, sigma),
        timing="host clock around mc_joint, seed list to per-rep counts; the legs alternate in one process after "
               "one warm-up round each; draw_ms_out: lb_joint_draw's event time (draw + LDPC encoder), the slower "
               "of the pipeline's two slices",
        settings=[],
    )
    for name, kw in (("default (fp64 AMP, reference LLR, sumprod2)", dict(precision="fp64")),
                     ("precision=fp32, llr=two_sided", dict(precision="fp32", llr="two_sided"))):
        jd = joint.joint_decoder(L, M, N_SPARC, lp, T, **kw)
        out["settings"].append(setting(name, jd, Pl, sigma, args.rounds, args.batch, args.soft_iter))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
