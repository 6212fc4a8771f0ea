#!/usr/bin/env python
"""Check the words of tests/ldpc_fixed_cases.py on the CPU, from the NumPy
statement of the fixed-point decoder alone (tests/ldpc_fixed_ref.py), and choose
the seeds it adds (EXTRA_AWGN): per cell, at the default widths and corr_factor
0.75, the words must stop after 0 sweeps, after 1..3, after 4..11 and run out at
12.  Where the layered tests' words leave a class empty, the first (sigma, seed)
of an AWGN word that fills it is printed as a Python literal.  Also prints each
cell's sweep counts and clip events at every widths, and whether the pin words
fire any clip at (2, 8, 16) and (3, 8, 16).

    python scripts/ldpc_fixed_case_seeds.py [cell ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ldpc_cases as lc  # noqa: E402
import ldpc_fixed_cases as qc  # noqa: E402
import ldpc_fixed_ref as qr  # noqa: E402

SIGMAS = np.round(np.arange(0.30, 1.30, 0.04), 2)
CLASSES = {"0": (0, 0), "1..3": (1, 3), "4..11": (4, qc.K_TRACE - 1), "12": (qc.K_TRACE, qc.K_TRACE)}


def sweeps(cell, ch):
    return qr.decode(ch, None, None, None, None, *qr.DEFAULT, corr_factor=0.75, max_it=qc.K_TRACE,
                     layers=qc.layers(cell))[1]


def missing(its):
    return [name for name, (lo, hi) in CLASSES.items() if not any(lo <= it <= hi for it in its)]


def choose(cell):
    c = qc.make_code(cell)
    labels, CH = qc.words(cell, c, extra=False)
    its = [sweeps(cell, ch) for ch in CH]
    print(f"# {cell}: {dict(zip(range(len(its)), zip(labels, its)))}", file=sys.stderr)
    out = []
    for name in missing(its):
        lo, hi = CLASSES[name]
        found = next(((float(sigma), seed) for seed in range(40) for sigma in SIGMAS
                      if lo <= sweeps(cell, lc.awgn_word(c, float(sigma), seed)[1]) <= hi), None)
        if found is None:
            raise RuntimeError(f"{cell}: no AWGN word that stops after {name} sweeps")
        out.append(found)
    return out


if __name__ == "__main__":
    cells = sys.argv[1:] or list(qc.CELLS)
    extra = {cell: choose(cell) for cell in cells}
    print("EXTRA_AWGN = {")
    for cell, found in extra.items():
        if found:
            print(f"    {cell!r}: {found!r},")
    print("}")
    for cell in cells:
        for widths in qc.WIDTHS:
            ref = qc.reference(cell, widths)
            print(f"# {cell} {widths}: sweeps {ref.its.tolist()} clips {ref.clips}")
        g = qc.layers(cell)
        for widths in (qc.PIN_WIDTHS, (3, 8, 16)):
            clips = {}
            its = [qr.decode(ch, None, None, None, None, *widths, corr_factor=1.0, max_it=qc.PIN_SWEEPS, layers=g,
                             clips=clips)[1] for ch in qc.pin_words(cell)]
            print(f"# {cell} pin words {widths}: sweeps {its} clip events {sum(clips.values())}")
        qc.check_preconditions(cell)
