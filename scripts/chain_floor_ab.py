#!/usr/bin/env python3
"""Kernel-argument preload, priced on the bare two-kernel chain.

Builds scripts/chain_floor.hip twice from the one source, without and with
`-mllvm -amdgpu-kernarg-preload-count=16`, runs `chain_floor preload` of both
builds interleaved (one process per run) and prints, per mode and argument
form, the us per iteration of every run with min / mean / max per build.

The struct and wide forms compile to the same code in both builds: their
difference between the builds is the probe's own run-to-run range.  The head
form differs by the preload alone.

  python scripts/chain_floor_ab.py [--rounds 6] [--inner 2] > profiles/rNN_c2_chain_floor.txt
"""
import argparse
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "chain_floor.hip")
BUILDS = {
    "plain": (os.path.join(HERE, "chain_floor"), []),
    "preload": (os.path.join(HERE, "chain_floor_preload"), ["-mllvm", "-amdgpu-kernarg-preload-count=16"]),
}
MODES = {"0": "empty", "1": "data", "2": "data+Ab-table rows", "6": "section kernel only",
         "2x2": "data+Ab-table rows, two chains in flight: us per iteration of both"}
FORMS = ("struct", "wide", "head")
LINE = re.compile(r"round (\d+) mode (\w+): struct ([\d.]+) \| wide ([\d.]+) \| head ([\d.]+)")


def build():
    for exe, flags in BUILDS.values():
        if os.path.exists(exe) and os.path.getmtime(exe) >= os.path.getmtime(SRC):
            continue
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", *flags, "-o", exe, SRC], check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6, help="interleaved runs per build")
    ap.add_argument("--inner", type=int, default=2, help="rounds inside each run")
    a = ap.parse_args()
    build()
    # runs[build][mode][form] = [us per iteration, ...]
    runs = {b: {m: {f: [] for f in FORMS} for m in MODES} for b in BUILDS}
    for r in range(a.rounds):
        for b in (("plain", "preload") if r % 2 == 0 else ("preload", "plain")):
            out = subprocess.run([BUILDS[b][0], "preload", str(a.inner)], check=True, timeout=120,
                                 capture_output=True, text=True).stdout
            got = LINE.findall(out)
            if len(got) != a.inner * len(MODES):
                sys.exit(f"{b}: unexpected output\n{out}")
            for _, m, *v in got:
                for f, x in zip(FORMS, v):
                    runs[b][m][f].append(float(x))
    print(f"us per iteration, {a.rounds} interleaved runs per build x {a.inner} rounds per run "
          "(64 iterations per graph replay, median of 21 replays each)")
    for m, name in MODES.items():
        print(f"\nmode {m} ({name})")
        for f in FORMS:
            st = {}
            for b in BUILDS:
                v = runs[b][m][f]
                st[b] = (min(v), sum(v) / len(v), max(v))
                print(f"  {f:6s} {b:7s} " + " ".join(f"{x:.3f}" for x in v)
                      + f" | min {st[b][0]:.3f} mean {st[b][1]:.3f} max {st[b][2]:.3f}")
            d = st["preload"][1] - st["plain"][1]
            rng = max(st["plain"][2] - st["plain"][0], st["preload"][2] - st["preload"][0])
            print(f"  {f:6s} preload - plain {d:+.3f} us ({100 * d / st['plain'][1]:+.2f} %), "
                  f"widest min-max range of the two {rng:.3f} us")


if __name__ == "__main__":
    main()
