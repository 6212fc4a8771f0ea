#!/usr/bin/env python3
"""What a joint SPARC + LDPC step costs on a coupled design, and what it buys
(recorded, nothing asserted).

Shape: L = M = 512, the 802.16 rate-5/6 code with z = 192 (N = 4608: ns = 512,
l0 = 0, every section protected), base matrix (omega = 4, Lambda = 16): R = 19,
C = 16, n = 4617, P = 15, binary64, the `soft` exchange with soft_iter = 2,
B = 256 reps of seeds 0..255, T iterations a decode at the most (--T).

Timing.  Two legs, alternated: sc_joint.CoupledJointDecoder with the flat
allocation, and joint.JointDecoder (one decoder, not pipelined) at the same
(L, M, n) with the same allocation.  One warm-up of each, then --rounds rounds;
medians and ranges.  A step is split into
  amp    the three decodes' loops           device events (sa_sc_event_ms / sa_run_event_ms)
  start  A beta_0 and k_scstart, the two restarts' (coupled leg only; a run of T = 0
         from the staged beta, measured behind the step; it is part of amp)   device events
  bp     the two BP calls                    device events (lb_run_event_ms)
  glue   llr, hard indices, soft beta_0      end to end (the calls block; host time)
  step   the whole decode_staged             end to end (host time)

Payoff.  At each --sigmas the bit error rates after the first AMP, after the
first LDPC call and after the restart (and the second round's), over the same
256 seeds: the coupled design with the flat allocation against the uncoupled
decoder with pa_iterative (--rpa the rate it is built for).

Prints one JSON line and writes it to results/sc_joint.json (or --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=list(v))


def timed_soft_step(jd, B, T, soft_iter, amp_ms):
    """JointDecoder.decode_staged's soft branch, step by step, with its parts timed.  -> dict of ms."""
    op, l0, ns = jd.op, jd.l0, jd.ns
    t = dict(amp=0.0, bp=0.0, glue=0.0)
    w0 = time.perf_counter()
    op.run(B, T)
    op.wait()
    t["amp"] += amp_ms(op)
    op.decide(B)
    for _ in range(soft_iter):
        g0 = time.perf_counter()
        d_ch, d_app, _ = jd.code.device_buffers(B)
        op.llr(B, l0, ns, out=d_ch, **jd._llr_kw)
        t["glue"] += (time.perf_counter() - g0) * 1e3
        jd.code.run_buffers(B, **jd._bp_kw)
        t["bp"] += jd.code.mc_event_ms()
        g0 = time.perf_counter()
        op.hard_cancel(B, l0, ns, d_app)
        op.soft_beta0(B, l0, ns, d_app)
        t["glue"] += (time.perf_counter() - g0) * 1e3
        op.run(B, T, beta0=True)
        op.wait()
        t["amp"] += amp_ms(op)
        op.decide(B)
    t["step"] = (time.perf_counter() - w0) * 1e3
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "sc_joint.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=1.8)
    ap.add_argument("--sigmas", type=float, nargs="*", default=[1.7, 1.8, 1.9])
    ap.add_argument("--rpa", type=float, default=None, help="pa_iterative's rate (default: the design's)")
    ap.add_argument("--precision", default="fp64")
    args = ap.parse_args()
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd.joint import mc_joint

    L = M = 512
    omega, Lam, P, z = 4, 16, 15.0, 192
    W = sp.base_matrix(omega, Lam)
    R, C = W.shape
    n = R * 243
    B, T = args.reps, args.T
    flat = np.full(L, P / L)
    code_c = sp.code("802.16", "5/6", z)
    code_u = sp.code("802.16", "5/6", z)
    cjd = sp.CoupledJointDecoder(L, M, n, W, code_c, T, precision=args.precision)
    ujd = sp.JointDecoder(L, M, n, code_u, T, precision=args.precision)
    rate = L * np.log2(M) / n
    out = dict(workload=f"L={L} M={M} n={n} 802.16 5/6 z={z} (ns={cjd.ns}, l0={cjd.l0}) omega={omega} Lambda={Lam} R={R} C={C} "
                        f"P={P} B={B} T={T} {args.precision} soft x 2, seeds 0..{B - 1}",
               units=dict(amp="device events, ms", start="device events, ms (part of amp)", bp="device events, ms",
                          glue="end to end, host ms", step="end to end, host ms"),
               rounds=args.rounds, timing={}, payoff=[])

    seeds = list(range(B))
    idx, noise = cjd.draw([np.random.RandomState(s) for s in seeds], B, args.sigma)
    legs = dict(coupled=(cjd, lambda op: op.last_amp_ms()), uncoupled=(ujd, lambda op: op.last_run_ms()))

    def one(name):
        jd, amp_ms = legs[name]
        jd.stage(idx, noise, flat)
        t = timed_soft_step(jd, B, T, 2, amp_ms)
        if name == "coupled":  # the start alone: a run of no iterations from the beta on the device, twice a step
            jd.op.run(B, 0, beta0=True)
            jd.op.wait()
            t["start"] = 2 * jd.op.last_amp_ms()
        return t

    for name in legs:
        one(name)  # warm-up
    ms = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            ms[name].append(one(name))
    for name in legs:
        out["timing"][name] = {k: stats([r[k] for r in ms[name]]) for k in ms[name][0]}
    out["timing"]["coupled_over_uncoupled_step"] = (out["timing"]["coupled"]["step"]["median"] /
                                                     out["timing"]["uncoupled"]["step"]["median"])

    rpa = rate if args.rpa is None else args.rpa
    tb = cjd.total_bits
    for sigma in args.sigmas:
        pa = sp.pa_iterative(L, 32, sigma, P, rpa)
        row = dict(sigma=sigma, seeds=B, total_bits=tb, pa_iterative_rate=rpa)
        for name, jd, Pl in (("coupled_flat", cjd, flat), ("uncoupled_pa_iterative", ujd, pa), ("uncoupled_flat", ujd, flat)):
            r = mc_joint(jd, Pl, sigma, seeds, "soft", 2, batch=B, pipeline=False)
            row[name] = dict(ber_amp_1=float(r["amp"][:, 0].mean()) / tb, ber_ldpc_1=float(r["ldpc"][:, 0].mean()) / tb,
                             ber_amp_2=float(r["amp"][:, 1].mean()) / tb, ber_ldpc_2=float(r["ldpc"][:, 1].mean()) / tb,
                             ber_amp_3=float(r["amp"][:, 2].mean()) / tb,
                             blocks_in_error_after_restart=int((r["amp"][:, 1] > 0).sum()))
        out["payoff"].append(row)

    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
