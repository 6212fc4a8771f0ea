#!/usr/bin/env python3
"""Record the reps of tests/sc_joint_cases.py from the NumPy statement alone
(tests/sc_joint_ref.py; no GPU): per joint case, per seed of SCAN and per mode
(soft with soft_iter = 2, hard) the statement's counts (amp, ldpc), BP iteration
counts, AMP stop indices, the smallest BP stop margin and the smallest top-two
gap, and whether the rep is an exact-count rep:

  * every BP call stops in [0, 199] (none runs its 200 iterations),
  * the smallest stop margin of any BP call is >= MIN_BP_MARGIN = 1e-3,
  * the smallest top-two gap of any estimate is >= MIN_GAP = 1e-6 (of c_l),
  * every BP call of the statement returns the same iteration count when its
    input LLRs are moved by LLR_PERTURB = 1e-9 relative (PERTURB_DRAWS = 4 sign
    patterns from RandomState(1000 + seed)): 1e-9 is what the device's LLRs are
    held to against the reference's (tests/test_gpu_joint.py), and a long BP
    call amplifies it (K3L seed 2: 100 iterations unperturbed, 79 to 110
    perturbed, every margin above the floor);

the floors and the perturbation are reasoned in tests/sc_joint_cases.py.  Nothing is discarded: the
reps that are not exact feed the forced-input test.  The script then checks
the table's condition: K1, K2 and K3 each keep at least two seeds, and K0 at
least one, that are exact in both modes, with (K1-K3) bit errors after the
first AMP and, in every one, a BP call of at least one iteration.

    python scripts/sc_joint_case_seeds.py [--write]

prints the table; --write replaces the RECORDED block of tests/sc_joint_cases.py.
"""
import argparse
import os
import pprint
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sc_joint_cases as jc  # noqa: E402
import sc_joint_ref as ref  # noqa: E402

BEGIN = "# --- recorded by scripts/sc_joint_case_seeds.py: begin ---\n"
END = "# --- recorded by scripts/sc_joint_case_seeds.py: end ---\n"


def look(case, seed, mode):
    r = ref.joint_rep(case, jc.graph(), seed, mode, jc.SOFT_ITER, jc.T, max_it=jc.MAX_IT)
    its = [int(i) for i in r["bp_iters"]]
    exact = all(0 <= i < jc.MAX_IT for i in its) and r["bp_margin"] >= jc.MIN_BP_MARGIN and r["gap"] >= jc.MIN_GAP
    stable = True
    if exact:  # the statement's own BP calls on LLRs moved by what the device's may differ by
        rs = np.random.RandomState(1000 + seed)
        for llr, it in zip(r["llrs"], its):
            for _ in range(jc.PERTURB_DRAWS):
                moved = llr * (1.0 + jc.LLR_PERTURB * rs.choice([-1.0, 1.0], llr.size))
                stable = stable and jc.graph().decode(moved, jc.MAX_IT)[1] == it
    exact = exact and stable
    return dict(bp_stable=bool(stable), amp=[int(v) for v in r["amp"]], ldpc=[int(v) for v in r["ldpc"]], bp_iters=its,
                stops=[int(v) for v in r["stops"]], bp_margin=float(f"{r['bp_margin']:.4g}"), gap=float(f"{r['gap']:.4g}"),
                exact=bool(exact))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    rec = {}
    for case in jc.JOINT_CASES:
        rec[case.name] = {}
        for seed in jc.SCAN:
            rec[case.name][seed] = {m: look(case, seed, m) for m in jc.MODES}
            for m in jc.MODES:
                d = rec[case.name][seed][m]
                print(f"{case.name} sigma {case.sigma} seed {seed:2d} {m:4s}: amp {d['amp']} ldpc {d['ldpc']} bp {d['bp_iters']} "
                      f"stops {d['stops']} margin {d['bp_margin']:.3g} gap {d['gap']:.3g} {'exact' if d['exact'] else '-'}"
                      f"{'' if d['bp_stable'] else ' (BP count moves under the LLR perturbation)'}")
    for case in jc.JOINT_CASES:
        good = [s for s in jc.SCAN if all(rec[case.name][s][m]["exact"] and max(rec[case.name][s][m]["bp_iters"]) >= 1
                                          for m in jc.MODES)]
        hit = [s for s in good if rec[case.name][s]["soft"]["amp"][0] > 0]
        print(f"{case.name}: exact in both modes with a BP call of >= 1 iteration: {good}; of them with first-AMP errors: {hit}")
        if case.name in ("K1", "K2", "K3"):
            assert len(hit) >= 2, f"{case.name} keeps fewer than two such seeds"
        if case.name == "K0":
            assert len(good) >= 1, "K0 keeps no such seed"
    if args.write:
        path = os.path.join(ROOT, "tests", "sc_joint_cases.py")
        with open(path) as fh:
            txt = fh.read()
        a, b = txt.index(BEGIN) + len(BEGIN), txt.index(END)
        txt = txt[:a] + "RECORDED = " + pprint.pformat(rec, width=150, compact=True, sort_dicts=False) + "\n" + txt[b:]
        with open(path, "w") as fh:
            fh.write(txt)
        print("wrote", path)


if __name__ == "__main__":
    np.seterr(all="ignore")
    main()
