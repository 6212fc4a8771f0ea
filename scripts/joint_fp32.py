#!/usr/bin/env python3
"""The two measurements of DESIGN.md §10c (results/joint_fp32.json): the joint
decoder with the two-sided LLR and a chosen BP decoder against its default.

  throughput : scripts/bench_joint.py --no-cpu at its defaults (configs[4], 256
               codewords, soft x2) in four legs — the default (binary64,
               reference LLR, sumprod2), binary32 + two-sided LLR, the same
               with layered_sumprod2_f32, binary64 with layered_sumprod2 — a
               warm-up run of each, then --rounds interleaved rounds, the
               order reversed from round to round.
  fidelity   : scripts/waterfall.py --sweep soft on the same seeds for every
               run: binary64 and binary32, reference LLR and two-sided LLR
               with clip none / 40 / 25 / 15.

Every run is a process of its own under its own time limit; the script stops
at the first abnormal exit and rewrites --out after every run.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGS = [
    ("default", []),
    ("fp32_two_sided", ["--precision", "fp32", "--llr", "two_sided"]),
    ("fp32_two_sided_layered_f32", ["--precision", "fp32", "--llr", "two_sided", "--bp-dectype", "layered_sumprod2_f32"]),
    ("fp64_layered", ["--bp-dectype", "layered_sumprod2"]),
]
CLIPS = [None, 40, 25, 15]


def run(cmd, limit):
    t0 = time.time()
    p = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-2000:])
        sys.exit(f"{' '.join(cmd)}: exit status {p.returncode}; stopping")
    return p.stdout, time.time() - t0


def save(path, key, value):
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(doc, open(path, "w"), indent=1)


def throughput(args):
    bench = [os.path.join("scripts", "bench_joint.py"), "--no-cpu", "--steps", str(args.steps)]
    runs = []
    for r in range(-1, args.rounds):  # round -1: the warm-up run of each leg, not kept
        for name, extra in (LEGS if r % 2 == 0 else LEGS[::-1]):
            out, sec = run(bench + extra, args.limit)
            d = json.loads(out.strip().splitlines()[-1])
            print(f"round {r} {name:28s} {d['ms_per_step']:9.3f} ms/step {d['value']:9.1f} cw/s ({sec:.0f} s)", flush=True)
            if r < 0:
                continue
            bp = {k: d["bp"][k] for k in ("kernel", "launch_ms", "mean_iterations", "max_iterations")}
            runs.append({"leg": name, "round": r, "ms_per_step": d["ms_per_step"], "value": d["value"],
                         "step_share_ms": d["step_share_ms"], "bp": bp, "llr": d.get("llr"), "errors": d["errors"]})
            legs = {}
            for name2, extra2 in LEGS:
                v = [x["ms_per_step"] for x in runs if x["leg"] == name2]
                if v:
                    legs[name2] = {"args": " ".join(extra2), "ms_per_step_min": min(v), "ms_per_step_max": max(v)}
            base = legs.get("default")
            for name2, s in legs.items():  # the bar of an opt-in path: every round below every round of the default
                s["every_round_below_default"] = (base is not None and name2 != "default"
                                                  and s["ms_per_step_max"] < base["ms_per_step_min"])
            save(args.out, "throughput", {"command": "scripts/bench_joint.py --no-cpu --steps %d <leg args>" % args.steps,
                                          "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                                          "rounds": args.rounds, "legs": legs, "runs": runs})


def fidelity(args):
    base = [os.path.join("scripts", "waterfall.py"), "--sweep", "soft", "--points", str(args.points), "--batch",
            str(args.batch), "--min-errors", str(args.blocks), "--max-blocks", str(args.blocks), "--no-bpsk"]
    runs = []
    args.tmp = args.tmp or tempfile.mkdtemp(prefix="joint_fp32_")
    for prec in ("fp64", "fp32"):
        for llr, clip in [("reference", None)] + [("two_sided", c) for c in CLIPS]:
            tag = f"{prec}_{llr}" + ("" if llr == "reference" else f"_clip{clip or 'none'}")
            out_base = os.path.join(args.tmp, tag)
            extra = ["--precision", prec, "--llr", llr, "--out", out_base] + (["--llr-clip", str(clip)] if clip else [])
            os.makedirs(args.tmp, exist_ok=True)
            _, sec = run(base + extra, args.limit)
            rows = json.load(open(out_base + ".json"))["rows"]
            cols = ("EbN0_dB", "BER_amp_1", "BER_ldpc", "BER_amp_2", "BER_ldpc_2", "BER_plain", "blocks")
            runs.append({"run": tag, "precision": prec, "llr": llr, "clip": clip, "seconds": round(sec, 1),
                         "rows": [{k: r[k] for k in cols} for r in rows],
                         "published": [r["reference"] for r in rows]})
            print(f"{tag:28s} ({sec:.0f} s) BER_ldpc " + " ".join(f"{r['BER_ldpc']:.2e}" for r in rows), flush=True)
            save(args.out, "fidelity", {"command": "scripts/waterfall.py " + " ".join(base[1:]) + " <run args>",
                                        "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "runs": runs})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["throughput", "fidelity"])
    ap.add_argument("--out", default=os.path.join(ROOT, "results", "joint_fp32.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per run")
    ap.add_argument("--points", type=int, default=10, help="fidelity: Eb/N0 points of linspace(3, 10, 10)")
    ap.add_argument("--blocks", type=int, default=64, help="fidelity: blocks per point (MIN_ERRORS = MAX_BLOCKS)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tmp", default=None, help="fidelity: where the sweeps write (default: a temporary directory)")
    args = ap.parse_args()
    throughput(args) if args.what == "throughput" else fidelity(args)


if __name__ == "__main__":
    main()
