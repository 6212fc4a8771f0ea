#!/usr/bin/env python
"""Choose the word seeds and the sumprod2 bar of tests/ldpc_f32_cases.py (_SEEDS,
P_CELL, P_MEDIAN) on the CPU, from the NumPy reference alone
(tests/ldpc_f32_ref.py).

Per (cell, algorithm) and word kind, candidates are taken in a fixed order
(seed, then parameter) and kept when the reference's sweeps fit the kind (AWGN
words that stop after 1, after 3 and after >= 6 sweeps, a word that never
converges, ...).  A sumprod2 candidate is decoded twice, with c(x) = log(1 +
exp(-x)) in binary32 and correctly rounded, and must stop after the same sweeps
both times; its movement is the largest change of app between the two runs,
relative to max(1, |app|), through K_TRACE sweeps.

Then, over all cells at once: P = the largest movement of the chosen words,
B = 16 P.  A word that moves more than ten times the median, or one of whose
stop tests is a knife-edge at 100 B (ldpc_f32_cases.stop_margins: the smallest
non-zero |app| is under it and no check of odd parity has all its variables
above it), gives way to its kind's next candidate, the worst mover first,
until nothing changes.  The never-converging word is lc.hopeless_word where
one passes, else an AWGN word far below threshold (the confident words are
chaotic in binary32 on the rate-1/2 codes).  Prints the tables as Python
literals.

    python scripts/ldpc_f32_case_seeds.py [cell ...]
"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ldpc_cases as lc  # noqa: E402
import ldpc_f32_cases as fc  # noqa: E402
import ldpc_layered_ref as lr  # noqa: E402

SIGMAS = np.round(np.arange(0.30, 1.30, 0.04), 2)
KEEP = 48  # candidates kept per word kind


def candidates(job):
    """cell, algo -> {slot: [(params, it, smallest margin, movement), ...]} in candidate order."""
    cell, algo = job
    c = fc.make_code(cell)
    layers = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    keep = KEEP if algo == "sumprod2" else 1
    last = fc.K_TRACE - 1

    def measure(ch, fits):
        """(it, margin, movement) when the word fits its kind, else None."""
        it, apps, margins = fc.trace(c, ch, algo, layers)
        if not fits(it):
            return None
        if algo != "sumprod2":
            return it, float(np.min(margins)), 0.0
        it1, apps1, _ = fc.trace(c, ch, algo, layers, rounded=True)
        if it1 != it:
            return None
        return it, float(np.min(fc.stop_margins(layers, apps[:len(margins)], margins))), fc.movement(apps, apps1)

    out = {}
    ranges = [(1, 3), (4, last)] if cell in fc.TWO_WORDS else [(1, 1), (3, 3), (6, last)]
    for i, (lo_, hi) in enumerate(ranges):
        got = out.setdefault(("awgn", i), [])
        for seed in range(40):
            for sigma in SIGMAS:
                if len(got) >= keep:
                    break
                m = measure(lc.awgn_word(c, float(sigma), seed)[1], lambda it: lo_ <= it <= hi)
                if m:
                    got.append(((float(sigma), seed),) + m)
    if cell in fc.TWO_WORDS:
        return cell, algo, out

    def scan(name, params, make, fits, label=lambda par, seed: (par, seed) if par is not None else seed):
        got = out.setdefault((name, 0), [])
        for par in params:
            for seed in range(60 if len(params) < 8 else 8):
                if len(got) >= keep:
                    return
                m = measure(make(par, seed), fits)
                if m:
                    got.append((label(par, seed),) + m)

    # the never-converging word: lc.hopeless_word, then (its candidates are all ill-conditioned in
    # binary32 at rate 1/2) AWGN words far below the threshold
    never = [(f, None) for f in (0.12, 0.2, 0.3, 0.08)] + [(None, sg) for sg in (1.6, 2.0, 1.3, 2.5)]
    scan("hopeless", never,
         lambda par, sd: fc.never_converging_word(c, (par[0], sd) if par[1] is None else ("awgn", par[1], sd)),
         lambda it: it == fc.K_TRACE, lambda par, sd: (par[0], sd) if par[1] is None else ("awgn", par[1], sd))
    scan("gauss", (3.0, 6.0, 10.0, 15.0, 25.0), lambda sc, sd: sc * np.random.RandomState(sd).randn(c.N),
         lambda it: True)
    scan("erase", (0.6, 0.5, 0.42, 0.36, 0.3), lambda sg, sd: lc.erase_word(c, sg, sd), lambda it: it > 0)
    scan("sat", (None,), lambda _, sd: lc.sat_word(c, sd), lambda it: True)
    scan("clamp", (0.6, 0.5, 0.42), lambda sg, sd: fc.clamp_word(c, sg, sd), lambda it: True)
    return cell, algo, out


def select(table):
    """The first candidate of every slot, advanced past the words the global preconditions reject."""
    pick = {key: 0 for key in table}
    for key, cands in table.items():
        if not cands:
            raise RuntimeError(f"no candidate for {key}")
    while True:
        sp2 = {k: table[k][i] for k, i in pick.items() if k[1] == "sumprod2"}
        moves = np.array([v[3] for v in sp2.values()])
        median = float(np.median(moves[moves > 0]))
        P = float(moves.max())
        bad = [k for k, v in sp2.items() if v[3] > 10 * median or v[2] < 100 * 16 * P]
        if not bad:
            return pick, P, median
        # the worst offender gives way first: P may fall with it
        k = max(bad, key=lambda k: sp2[k][3])
        pick[k] += 1
        if pick[k] >= len(table[k]):
            raise RuntimeError(f"{k}: every candidate rejected ({table[k]})")
        print(f"# {k}: next candidate", file=sys.stderr)


if __name__ == "__main__":
    cells = sys.argv[1:] or list(fc.CELLS)
    jobs = [(cell, algo) for cell in cells for algo in fc.ALGOS]
    table = {}
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        for cell, algo, out in pool.imap_unordered(candidates, jobs):
            for (name, i), cands in out.items():
                table[(cell, algo, name, i)] = cands
            print(f"# {cell} {algo} done", file=sys.stderr, flush=True)
    pick, P, median = select(table)
    chosen = {k: table[k][i] for k, i in pick.items()}
    print("_SEEDS = {  # (awgn, hopeless, gauss, erase, sat, clamp)")
    for cell in cells:
        print(f"    {cell!r}: {{")
        for algo in fc.ALGOS:
            awgn = [chosen[k][0] for k in sorted(chosen) if k[:3] == (cell, algo, "awgn")]
            rest = tuple(chosen[(cell, algo, n, 0)][0] if (cell, algo, n, 0) in chosen else None for n in fc._KEYS[1:])
            print(f"        {algo!r}: {(awgn,) + rest!r},")
        print("    },")
    print("}")
    print("P_CELL = {")
    for cell in cells:
        print(f"    {cell!r}: {max(v[3] for k, v in chosen.items() if k[0] == cell and k[1] == 'sumprod2')!r},")
    print("}")
    print(f"P_MEDIAN = {median!r}")
    print(f"# P = {P!r}, B = {16 * P!r}, 100 B = {1600 * P!r}")
    for k in sorted(chosen):
        if k[1] == "sumprod2":
            print(f"# {k}: sweeps {chosen[k][1]}, smallest margin {chosen[k][2]:.3e}, movement {chosen[k][3]:.3e}")
