#!/usr/bin/env python3
"""Interleaved A/B rounds of library builds over one bench command, every run
in a process of its own under its own time limit; stops at the first abnormal
exit.  Each round runs every build once, the order reversed from round to
round.  Prints one line per run and appends the set to a JSON file.

  python scripts/ab_rounds.py --out results/ab.json --tag set1 --rounds 6 \
      parent=/path/libsparc_amp.so change= -- --steps 200 --warmup 20

NAME= (no path) is the in-tree build.  --lone times, instead of the bench, 50 x
(sa_run, sa_decide_async, sa_decide_collect) with nothing in flight beside it
(wall time per step, median of 5 repeats) at the bench's c2 shape.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LONE = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, %r)
import bench, sparc_ldpc_amd as sp
w = bench.WORKLOADS["c2"]
L, M, T = w["L"], w["M"], w["T"]
n = bench.n_of(w)
Pl = w["P"] / L * np.ones(L)
op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=sys.argv[1])
y = bench.synth_y(op, Pl, w["sigma"], [1000])
op.reserve(1, T)
op.stage(y, Pl)
def steps(k):
    for _ in range(k):
        op.run(1, T, early_stop=False)
        op.decide_async(1, 0)
        op.decide_collect(1, 0)
steps(10)
reps = []
for _ in range(5):
    op.wait()
    t0 = time.perf_counter()
    steps(50)
    reps.append((time.perf_counter() - t0) / 50 * 1e3)
print(json.dumps({"value": round(float(np.median(reps)), 5), "unit": "ms per lone step", "repeats": [round(r, 5) for r in reps]}))
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--tag", required=True)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--limit", type=int, default=150, help="seconds per run")
    ap.add_argument("--lone", default="", metavar="PRECISION")
    ap.add_argument("builds", nargs="+", help="NAME=LIB ... -- bench args")
    argv = sys.argv[1:]
    bench_args = argv[argv.index("--") + 1:] if "--" in argv else []
    args = ap.parse_args(argv[:argv.index("--")] if "--" in argv else argv)
    builds = [b.split("=", 1) for b in args.builds]
    cmd = ([sys.executable, "-c", LONE % ROOT, args.lone] if args.lone
           else [sys.executable, os.path.join(ROOT, "bench.py")] + bench_args)
    runs = []
    for r in range(args.rounds):
        for name, lib in (builds if r % 2 == 0 else builds[::-1]):
            env = dict(os.environ)
            env.pop("SPARC_AMP_LIB", None)
            if lib:
                env["SPARC_AMP_LIB"] = os.path.abspath(lib)
            p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=args.limit)
            if p.returncode != 0:
                print(p.stdout[-2000:], p.stderr[-2000:])
                sys.exit(f"{name} round {r}: exit status {p.returncode}; stopping")
            d = json.loads(p.stdout.strip().splitlines()[-1])
            runs.append({"build": name, "round": r, "value": d["value"], "unit": d["unit"],
                         **({"ms_per_step": d["ms_per_step"]} if "ms_per_step" in d else {})})
            print(f"{args.tag} round {r} {name:8s} {d['value']:.3f} {d['unit']}", flush=True)
    summary = {}
    for name, _ in builds:
        v = [x["value"] for x in runs if x["build"] == name]
        summary[name] = {"min": min(v), "max": max(v), "mean": round(sum(v) / len(v), 3)}
    print(json.dumps(summary))
    sets = json.load(open(args.out)) if os.path.exists(args.out) else []
    sets.append({"tag": args.tag, "utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                 "command": "lone steps, " + args.lone if args.lone else "bench.py " + " ".join(bench_args),
                 "runs": runs, "summary": summary})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(sets, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
