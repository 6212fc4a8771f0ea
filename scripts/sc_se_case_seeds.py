#!/usr/bin/env python
"""Choose the base seeds of tests/sc_se_cases.py (_CHOSEN) on the CPU, from the
NumPy statement of coupled state evolution alone (tests/sc_se_ref.py).  Per
case, the first base seed from 0 at which

  * every miss comparison (configuration, section, sample, iteration) has a
    relative margin of at least sc_se_cases.MARGIN, so that a rounding
    difference cannot flip a miss count, and
  * the statement in binary64 and in np.longdouble agree on every miss count
    and on every predicted stop index: the stop index is a bit-equality of two
    phi rows, and a seed at which the two precisions place it differently is
    one at which a device whose sums run in another order could as well;

and, at that seed, the largest gap between the two statements over phi, tau2,
x and E, from which the GPU tests take their tolerance
(sc_se_cases.TOL_FACTOR times it).

    python scripts/sc_se_case_seeds.py [--write] [case ...]

Prints the table as a Python literal; --write also puts it into
tests/sc_se_cases.py between its "chosen" markers.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sc_se_cases as sc  # noqa: E402


def choose(name):
    for seed in range(200):
        d = sc.statement(name, seed, margin=True)
        margin = min(r[6] for r in d)
        if margin < sc.MARGIN:
            continue
        ld = sc.statement(name, seed, longdouble=True)
        if all(np.array_equal(a[3], b[3]) and a[5] == b[5] for a, b in zip(d, ld)):
            break
        print(f"# {name}: seed {seed} rejected: the two precisions disagree on a miss count or a stop index",
              file=sys.stderr, flush=True)
    else:
        raise RuntimeError(f"{name}: no seed with margin >= {sc.MARGIN} and agreeing stop indices")
    gap = max(float(np.max(np.abs(a[i] - b[i]))) for a, b in zip(d, ld) for i in (0, 1, 2, 4))
    print(f"# {name}: seed {seed}, margin {margin:.3e}, gap {gap:.3e}, stop {[r[5] for r in d]}", file=sys.stderr, flush=True)
    return seed, gap


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--write"]
    names = args or list(sc.CASES)
    table = dict(sc._CHOSEN)
    for name in names:
        table[name] = choose(name)
    lines = ["_CHOSEN = {"] + [f"    {k!r}: {table[k]!r}," for k in sc.CASES if k in table] + ["}"]
    block = "\n".join(lines)
    print(block)
    if "--write" in sys.argv[1:]:
        path = os.path.join(ROOT, "tests", "sc_se_cases.py")
        with open(path) as fh:
            src = fh.read()
        src = re.sub(r"(# --- chosen: begin ---\n).*?(\n# --- chosen: end ---)", lambda m: m.group(1) + block + m.group(2),
                     src, flags=re.S)
        with open(path, "w") as fh:
            fh.write(src)
