#!/usr/bin/env python
"""Choose the word seeds of tests/ldpc_cases.py (SEEDS) on the CPU, from the
NumPy oracle alone: per (cell, algorithm) the AWGN words the oracle stops at
iterations 1, 3 and 8, and the first seeds of the other words for which the
tests' preconditions hold (every stop margin > 1e-6, sumprod finite).
Prints the table as a Python literal.

    python scripts/ldpc_case_seeds.py [cell ...]
"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ldpc_cases as lc  # noqa: E402
from oracle import ldpc_oracle as lo  # noqa: E402

SIGMAS = np.round(np.arange(0.30, 1.30, 0.04), 2)


def _trace(c, ch, algo):
    _, it, ta, tm = lo._decode(ch, c.vdeg, c.cdeg, c.intrlv, algo, max_it=lc.K_TRACE, trace=True)
    ok = bool(np.all((tm > lc.MARGIN))) and (algo != "sumprod" or bool(np.isfinite(ta).all()))
    return it, ok, tm


def _first(make, accept, what):
    for seed in range(60):
        r = make(seed)
        if accept(*r):
            return seed
    raise RuntimeError(f"no seed for {what}")


def choose(job):
    cell, algo = job
    c = lc.make_code(cell)
    want = {(2, 7): None, (9, 11): None} if cell in lc.TWO_WORDS else {(h, h): None for h in lc.HANDOFFS}
    for seed in range(40):
        for sigma in SIGMAS:
            if all(v is not None for v in want.values()):
                break
            it, ok, _ = _trace(c, lc.awgn_word(c, float(sigma), seed)[1], algo)
            for (lo_, hi), v in want.items():
                if v is None and ok and lo_ <= it <= hi:
                    want[(lo_, hi)] = (float(sigma), seed)
    if any(v is None for v in want.values()):
        raise RuntimeError(f"{cell} {algo}: no AWGN word for {want}")
    out = {"awgn": [want[k] for k in sorted(want)]}
    if cell in lc.TWO_WORDS:
        return cell, algo, out

    def run(ch):
        return _trace(c, ch, algo)

    def search(name, params, make, accept):
        for par in params:
            try:
                out[name] = (par, _first(lambda sd: run(make(par, sd)), accept, f"{cell} {algo} {name}"))
                return
            except RuntimeError:
                pass
        raise RuntimeError(f"{cell} {algo}: no {name} word")

    search("hopeless", (0.12, 0.2, 0.3, 0.08), lambda f, sd: lc.hopeless_word(c, f, sd),
           lambda it, ok, tm: ok and it == lc.K_TRACE)
    search("gauss", (3.0, 6.0, 10.0, 15.0, 25.0), lambda sc, sd: sc * np.random.RandomState(sd).randn(c.N),
           lambda it, ok, tm: ok)
    if algo != "sumprod":
        # an erased bit's checks have an aggregate of exactly zero (see Ref.check_preconditions)
        search("erase", (0.6, 0.5, 0.42, 0.36, 0.3), lambda sg, sd: lc.erase_word(c, sg, sd),
               lambda it, ok, tm: bool(np.all((tm > lc.MARGIN) | (tm == 0.0))))
        out["sat"] = _first(lambda sd: run(lc.sat_word(c, sd)), lambda it, ok, tm: ok, f"{cell} {algo} sat")
    return cell, algo, out


if __name__ == "__main__":
    cells = sys.argv[1:] or list(lc.CELLS)
    jobs = [(cell, algo) for cell in cells for algo in lc.ALGOS]
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        table = {}
        for cell, algo, out in pool.imap_unordered(choose, jobs):
            table.setdefault(cell, {})[algo] = out
            print(f"# {cell} {algo} done", file=sys.stderr, flush=True)
    print("_SEEDS = {  # (awgn, hopeless, gauss, erase, sat)")
    for cell in cells:
        print(f"    {cell!r}: {{")
        for algo in lc.ALGOS:
            o = table[cell][algo]
            print(f"        {algo!r}: {tuple(o.get(k) for k in ('awgn', 'hopeless', 'gauss', 'erase', 'sat'))!r},")
        print("    },")
    print("}")
