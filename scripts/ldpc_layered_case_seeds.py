#!/usr/bin/env python
"""Choose the word seeds of tests/ldpc_layered_cases.py (SEEDS, SIM_SIGMA) on
the CPU, from the NumPy references alone: per (cell, algorithm) the AWGN words
the layered reference stops after 1, after 3 and after >= 6 sweeps, and the
first seeds of the other words for which the tests' preconditions hold (every
stop test's smallest non-zero |app| >= MARGIN; the log and log1p variants of
Lxor stop after the same sweeps).  Prints the table as a Python literal, and
for sim_ldpc_mc's blocks 0..63 of 802.16 1/2 z=24 the bit errors flooding and
layered sumprod2 leave at a few sigmas.

    python scripts/ldpc_layered_case_seeds.py [cell ...]
"""
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ldpc_cases as lc  # noqa: E402
import ldpc_layered_cases as llc  # noqa: E402
import ldpc_layered_ref as lr  # noqa: E402
from oracle import ldpc_oracle as lo  # noqa: E402

SIGMAS = np.round(np.arange(0.30, 1.30, 0.04), 2)


def _first(make, accept, what):
    for seed in range(60):
        if accept(make(seed)):
            return seed
    raise RuntimeError(f"no seed for {what}")


def choose(job):
    cell, algo = job
    c = llc.make_code(cell)
    layers = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    last = llc.K_TRACE - 1
    want = {(1, 3): None, (4, last): None} if cell in llc.TWO_WORDS else {(1, 1): None, (3, 3): None, (6, last): None}
    for seed in range(40):
        for sigma in SIGMAS:
            if all(v is not None for v in want.values()):
                break
            ok, it = llc.acceptable(c, lc.awgn_word(c, float(sigma), seed)[1], algo, layers)
            for (lo_, hi), v in want.items():
                if v is None and ok and lo_ <= it <= hi:
                    want[(lo_, hi)] = (float(sigma), seed)
    if any(v is None for v in want.values()):
        raise RuntimeError(f"{cell} {algo}: no AWGN word for {want}")
    out = {"awgn": [want[k] for k in sorted(want)]}
    if cell in llc.TWO_WORDS:
        return cell, algo, out

    def search(name, params, make, accept):
        for par in params:
            try:
                out[name] = (par, _first(lambda sd: llc.acceptable(c, make(par, sd), algo, layers), accept,
                                         f"{cell} {algo} {name}"))
                return
            except RuntimeError:
                pass
        raise RuntimeError(f"{cell} {algo}: no {name} word")

    search("hopeless", (0.12, 0.2, 0.3, 0.08), lambda f, sd: lc.hopeless_word(c, f, sd),
           lambda r: r[0] and r[1] == llc.K_TRACE)
    search("gauss", (3.0, 6.0, 10.0, 15.0, 25.0), lambda sc, sd: sc * np.random.RandomState(sd).randn(c.N),
           lambda r: r[0])
    search("erase", (0.6, 0.5, 0.42, 0.36, 0.3), lambda sg, sd: lc.erase_word(c, sg, sd), lambda r: r[0] and r[1] > 0)
    out["sat"] = _first(lambda sd: llc.acceptable(c, lc.sat_word(c, sd), algo, layers), lambda r: r[0],
                        f"{cell} {algo} sat")
    return cell, algo, out


def sim_sigmas():
    """Bit errors of flooding and layered sumprod2 on sim_ldpc_mc's blocks 0..63 (host draws)."""
    from sparc_ldpc_amd import ldpc_mc
    c = lc.make_code("16_1/2_z24")
    layers = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    u, w = ldpc_mc._draw_blocks(range(64), c.K, c.N, "awgn")
    X = c.encode_batch(u)
    for sigma in (0.7, 0.75, 0.8, 0.85, 0.9):
        CH = (2.0 / sigma ** 2) * ((1.0 - 2.0 * X) + sigma * w)
        fl = sum(int(((lo.sumprod2(ch, c.vdeg, c.cdeg, c.intrlv)[0] < 0) != x).sum()) for ch, x in zip(CH, X))
        la = sum(int(((lr.decode_code(c, ch, "sumprod2", layers=layers)[0] < 0) != x).sum()) for ch, x in zip(CH, X))
        print(f"# sim sigma={sigma}: flooding {fl} bit errors, layered {la}")


if __name__ == "__main__":
    cells = sys.argv[1:] or list(llc.CELLS)
    jobs = [(cell, algo) for cell in cells for algo in llc.ALGOS]
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        table = {}
        for cell, algo, out in pool.imap_unordered(choose, jobs):
            table.setdefault(cell, {})[algo] = out
            print(f"# {cell} {algo} done", file=sys.stderr, flush=True)
    print("_SEEDS = {  # (awgn, hopeless, gauss, erase, sat)")
    for cell in cells:
        print(f"    {cell!r}: {{")
        for algo in llc.ALGOS:
            o = table[cell][algo]
            print(f"        {algo!r}: {tuple(o.get(k) for k in llc._KEYS)!r},")
        print("    },")
    print("}")
    sim_sigmas()
