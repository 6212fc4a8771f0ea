"""The case table of the coupled decoder's tolerance stop and frozen column
blocks (tests/sc_wave_ref.py; CPU statement and GPU tests): small shapes, the
tolerances, and per (case, seed) what the statement does in T = 40 iterations.

The seeds and the RECORDED block are written by scripts/sc_wave_case_seeds.py
from the statement alone: per case the first seeds from 0 whose float32 and
float64 runs agree on every live mask and on the stop index, whose margins
(sc_wave_ref) are all >= MIN_MARGIN in both runs, and that freeze at least one
block before the stop.  MIN_MARGIN = 0.02: the binary32 device is allowed about
7e-6 relative on phi (parity), which moves a ratio by
about 1.4e-5; 0.02 x the smallest tolerance used with it (0.01) = 2e-4 leaves an
order of magnitude.  The (1e-3, 1e-2) cases ask for MIN_MARGIN_FINE = 0.2: 0.2 x
1e-3 = 2e-4, the same distance.
"""
import numpy as np

import sc_cases

T = 40
MIN_MARGIN = 0.02
MIN_MARGIN_FINE = 0.2


class WaveCase:
    def __init__(self, name, case, stop_tol, freeze_tol, nseeds, min_margin=MIN_MARGIN):
        self.name, self.case = name, case
        self.stop_tol, self.freeze_tol = stop_tol, freeze_tol
        self.nseeds, self.min_margin = nseeds, min_margin

    @property
    def seeds(self):
        return tuple(sorted(RECORDED.get(self.name, {})))

    def recorded(self, seed):
        return RECORDED[self.name][seed]


# the long chain: R = 17, n_r = 20, L_c = 4 (whole groups, the parent's Ab table)
LONG = sc_cases.Case("LONG", 64, 32, 340, 2, 16, 2.5, 0.5, ())
# the padded-group chain: L_c = 3, so each block's only group has an absent section
PAD = sc_cases.Case("PAD", 60, 16, 264, 3, 20, 3.0, 0.55, ())
# W = [[1]] on sc_cases.FLAT's shape: one block, frozen or live as a whole
FLAT = sc_cases.Case("FLAT", sc_cases.FLAT["L"], sc_cases.FLAT["M"], sc_cases.FLAT["n"], 1, 1, sc_cases.FLAT["P"],
                     sc_cases.FLAT["sigma"], ())

WAVE_CASES = (
    WaveCase("D", sc_cases.D, 0.01, 0.05, 2),
    WaveCase("LONG", LONG, 0.01, 0.05, 2),
    WaveCase("PAD", PAD, 0.01, 0.05, 1),
    WaveCase("C", sc_cases.C, 0.01, 0.05, 1),   # L_c = 5: a block spans two groups, one of them padded
    WaveCase("FLAT", FLAT, 0.01, 0.05, 1),
    WaveCase("LONG_FINE", LONG, 1e-3, 1e-2, 1, MIN_MARGIN_FINE),
)
BY_NAME = {w.name: w for w in WAVE_CASES}

# name -> seed -> stop index, frozen block-iterations before the stop, unfreeze
# events, and the smallest margin of the float32 and of the float64 run
# --- recorded by scripts/sc_wave_case_seeds.py: begin ---
RECORDED = {'D': {0: {'stop': 7, 'frozen': 7, 'total': 56, 'unfreeze': 2, 'margin32': 0.110262, 'margin64': 0.110261},
       1: {'stop': 6, 'frozen': 2, 'total': 48, 'unfreeze': 1, 'margin32': 0.135662, 'margin64': 0.135694}},
 'LONG': {2: {'stop': 18, 'frozen': 154, 'total': 288, 'unfreeze': 13, 'margin32': 0.044271, 'margin64': 0.044365},
          3: {'stop': 11, 'frozen': 70, 'total': 176, 'unfreeze': 10, 'margin32': 0.082549, 'margin64': 0.082559}},
 'PAD': {1: {'stop': 8, 'frozen': 23, 'total': 160, 'unfreeze': 4, 'margin32': 0.064466, 'margin64': 0.064465}},
 'C': {0: {'stop': 4, 'frozen': 3, 'total': 12, 'unfreeze': 0, 'margin32': 0.028168, 'margin64': 0.028202}},
 'FLAT': {9: {'stop': 12, 'frozen': 1, 'total': 12, 'unfreeze': 1, 'margin32': 0.309723, 'margin64': 0.30972}},
 'LONG_FINE': {6: {'stop': 7, 'frozen': 15, 'total': 112, 'unfreeze': 0, 'margin32': 0.276966, 'margin64': 0.276716}}}
# --- recorded by scripts/sc_wave_case_seeds.py: end ---

# every (wave case, seed) of the table
TABLE = [(w, s) for w in WAVE_CASES for s in w.seeds]
