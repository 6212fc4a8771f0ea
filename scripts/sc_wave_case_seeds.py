#!/usr/bin/env python3
"""Pick the seeds of tests/sc_wave_cases.py from the NumPy statement alone
(tests/sc_wave_ref.py; no GPU): per wave case the first seeds from 0 that

  * give equal live masks and equal stop indices in the float32 and the
    float64 run of the statement,
  * keep every margin of both runs at or above the case's min_margin,
  * freeze at least one block before the stop,

and record for each its stop index, frozen block-iterations, unfreeze events
and the two margins.  Prints every seed it looked at with the reason it was
passed over; --write replaces the RECORDED block of tests/sc_wave_cases.py.

    python scripts/sc_wave_case_seeds.py [--write] [--max-seed 64]
"""
import argparse
import os
import pprint
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sc_wave_cases as wc  # noqa: E402
import sc_wave_ref as ref  # noqa: E402

BEGIN = "# --- recorded by scripts/sc_wave_case_seeds.py: begin ---\n"
END = "# --- recorded by scripts/sc_wave_case_seeds.py: end ---\n"


def look(w, seed):
    """-> (record, None) for a seed that meets the rules, (record, reason) for one that does not."""
    c = w.case
    _, y = c.rep(seed)
    run = {}
    for dt in (np.float32, np.float64):
        _, stop, _, live, _, margin = ref.amp_sc_wave(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, w.stop_tol, w.freeze_tol, dtype=dt)
        run[dt] = (stop, live, margin)
    (s32, l32, m32), (s64, l64, m64) = run[np.float32], run[np.float64]
    frozen, total = ref.frozen_count(l64, s64)
    rec = dict(stop=s64, frozen=frozen, total=total, unfreeze=ref.unfreeze_events(l64, s64),
               margin32=round(m32, 6), margin64=round(m64, 6))
    if s32 != s64 or not np.array_equal(l32, l64):
        return rec, "float32 and float64 disagree"
    if min(m32, m64) < w.min_margin:
        return rec, f"margin {min(m32, m64):.4f} below {w.min_margin}"
    if frozen == 0:
        return rec, "nothing frozen before the stop"
    return rec, None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="replace the RECORDED block of tests/sc_wave_cases.py")
    ap.add_argument("--max-seed", type=int, default=64)
    args = ap.parse_args()
    recorded = {}
    for w in wc.WAVE_CASES:
        got = {}
        for seed in range(args.max_seed):
            rec, why = look(w, seed)
            print(f"{w.name:10s} seed {seed:2d}: {rec}  {'taken' if why is None else 'passed over: ' + why}")
            if why is None:
                got[seed] = rec
                if len(got) == w.nseeds:
                    break
        if len(got) < w.nseeds:
            sys.exit(f"case {w.name}: {len(got)} of {w.nseeds} seeds below {args.max_seed}")
        recorded[w.name] = got
    text = "RECORDED = " + pprint.pformat(recorded, width=118, sort_dicts=False) + "\n"
    print(text)
    if args.write:
        path = os.path.join(ROOT, "tests", "sc_wave_cases.py")
        with open(path) as fh:
            src = fh.read()
        pat = re.compile(re.escape(BEGIN) + ".*?" + re.escape(END), re.S)
        assert len(pat.findall(src)) == 1, "the RECORDED block's markers"
        with open(path, "w") as fh:
            fh.write(pat.sub(lambda m: BEGIN + text + END, src))
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
