#!/usr/bin/env python
"""Choose the base seeds of tests/se_cases.py (_CHOSEN) on the CPU, from the
NumPy statement of state evolution alone (tests/se_ref.py).  Per case: the
first base seed from 0 at which every miss comparison (allocation, section,
sample, iteration) has a relative margin of at least se_cases.MARGIN, so that a
rounding difference cannot flip a miss count; and, at that seed, the largest gap
between the statement in binary64 and in np.longdouble over tau2 and x, from
which the GPU tests take their tolerance (se_cases.TOL_FACTOR times it).

    python scripts/se_case_seeds.py [--write] [case ...]

Prints the table as a Python literal; --write also puts it into
tests/se_cases.py between its "chosen" markers.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import se_cases as sc  # noqa: E402


def choose(name):
    for seed in range(200):
        t2, x, _, _, margin = sc.statement(name, seed, margin=True)
        if margin >= sc.MARGIN:
            break
    else:
        raise RuntimeError(f"{name}: no seed with margin >= {sc.MARGIN}")
    t2l, xl, _, _ = sc.statement(name, seed, longdouble=True)
    gap = max(float(np.max(np.abs(t2 - t2l))), float(np.max(np.abs(x - xl))))
    print(f"# {name}: seed {seed}, margin {margin:.3e}, gap {gap:.3e}", file=sys.stderr, flush=True)
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
        path = os.path.join(ROOT, "tests", "se_cases.py")
        with open(path) as fh:
            src = fh.read()
        src = re.sub(r"(# --- chosen: begin ---\n).*?(\n# --- chosen: end ---)", lambda m: m.group(1) + block + m.group(2),
                     src, flags=re.S)
        with open(path, "w") as fh:
            fh.write(src)
