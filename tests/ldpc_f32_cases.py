"""Shared inputs of the binary32 layered belief-propagation tests (no tests
here): the cells that reach every k_bpl32 instance and layout, their seeded
words, the NumPy reference's traced decodes (tests/ldpc_f32_ref.py) and the bar
of the sumprod2 comparison.  Test infrastructure only: the product never
imports this module."""
import functools

import numpy as np

import ldpc_cases as lc
import ldpc_f32_ref as fr
import ldpc_layered_cases as llc
import ldpc_layered_ref as lr

KS = llc.KS  # max_iter of the truncated decodes
K_TRACE = llc.K_TRACE
ALGOS = fr.ALGOS
TWO_WORDS = llc.TWO_WORDS
make_code = llc.make_code
DBL_MAX = float(np.finfo(np.float64).max)

# name -> what layer_info("f32") must report: (lds_messages, max_layer, threads, lds_bytes, resident)
#   lds_bytes = 4 (Nv + Nmsg) with r and app in LDS, 4 Nv with app alone.
#   resident: workgroups a CU holds, the least of 160 KB / lds_bytes, 2048 threads a CU / threads, and what the
#   instance's registers allow (8 waves per SIMD up to 64 VGPRs: DCMAX 8 and 16; 6 at 80: DCFIX 20; 5 at 88: DCMAX 32).
CELLS = {
    "16_1/2_z24": (2, 24, 192, 4 * (576 + 1824), 10),  # DCMAX=8, irregular dc 6/7
    "11n_1/2_z27": (2, 27, 256, 4 * (648 + 2376), 8),  # dv up to 12
    "16_5/6_z24": (2, 24, 512, 4 * (576 + 1920), 3),  # DCFIX=20
    "syn_dc8": (2, 8, 128, 4 * (128 + 376), 16),  # checks of degree 2 and 3
    "syn_dc32": (2, 8, 256, 4 * (320 + 1056), 5),  # DCMAX=32
    "16_1/2_z96": (2, 96, 704, 4 * (2304 + 7296), 2),  # 672 edges a layer
    "16_5/6_z192": (2, 192, 768, 4 * (4608 + 15360), 2),  # the 78 KB image: two workgroups a CU
    "16_5/6_z300": (2, 300, 768, 4 * (7200 + 24000), 1),  # binary64 keeps r in HBM here: the element size decides
    "16_5/6_z864": (1, 864, 768, 4 * 20736, 1),  # app in LDS, r in HBM (as floats in the message slices)
}

# The sumprod2 bar, from the reference alone (scripts/ldpc_f32_case_seeds.py).  Every chosen word is
# decoded twice through K_TRACE sweeps: with c(x) = log(1 + exp(-x)) in binary32 by NumPy's float32
# exp / log (the statement), and with c in binary64 rounded once (correctly rounded).  P_CELL: the
# largest movement of app between the two, relative to max(1, |app|), over the cell's words and sweeps.
# P: the largest of them.  B = 16 P (rtol = atol) is the device's bar: v_exp_f32 / v_log_f32 may carry
# a few ulp where NumPy's routines carry about one (a factor up to 8), doubled for slack.
# P_MEDIAN: the median over the words that move at all; no word may move more than 10 P_MEDIAN.
P_CELL = {
    '16_1/2_z24': 6.0602669305172215e-06,
    '11n_1/2_z27': 2.86102294921875e-06,
    '16_5/6_z24': 9.715557098388672e-06,
    'syn_dc8': 9.5367431640625e-06,
    'syn_dc32': 2.86102294921875e-06,
    '16_1/2_z96': 2.468233830600176e-06,
    '16_5/6_z192': 2.48111622441597e-06,
    '16_5/6_z300': 5.364418029785156e-06,
    '16_5/6_z864': 4.76837158203125e-06,
}
P_MEDIAN = 1.0686459699864368e-06
P = max(P_CELL.values())
B = 16 * P
# No knife-edge stop decision: at every stop test of a chosen word either the smallest non-zero |app|
# is at least MARGIN (no hard decision can differ on the device), or the test fails whatever the
# variables under MARGIN decide: some check whose variables all have |app| >= MARGIN has odd parity.
# (The second case admits words that never converge.  In binary32 the window between 100 B and the
# smallest of a few thousand |app| values is too narrow for them otherwise: B cannot be under
# 16 * 2^-24 * the amplification of 12 sweeps, about 1e-4, and a never-converging word's smallest
# |app| over 13 stop tests is about 1e-3.)
MARGIN = 100 * B
# NumPy's float32 exp and log differ in the last place between CPU families (its SIMD kernels), so a
# word's movement measured where the tests run may differ from the recorded one: the tests hold it
# to twice the recorded bound (ill-conditioned words move by decades, not by a factor), B stays fixed.
P_RECHECK = 2.0

# Seeds chosen on the CPU from the NumPy reference alone (scripts/ldpc_f32_case_seeds.py): per (cell, algorithm)
#   "awgn": (sigma, seed) of the words the reference stops after 1, after 3 and after >= 6 sweeps
#           (TWO_WORDS cells: one word stopping after 1..3 sweeps, one after >= 4),
#   "hopeless": the never-converging word: (share of wrong signs, seed) of lc.hopeless_word, or
#               ("awgn", sigma, seed), an AWGN word far below the code's threshold, where every
#               hopeless_word is ill-conditioned in binary32 (the rate-1/2 codes: confident contradictory
#               inputs make the sweeps chaotic, a last-place difference grows threefold a sweep),
#   "gauss": (scale, seed), "erase": (sigma, seed), "sat": seed, "clamp": (sigma, seed).
_SEEDS = {  # (awgn, hopeless, gauss, erase, sat, clamp)
    '16_1/2_z24': {
        'sumprod2': ([(0.38, 0), (0.62, 0), (0.82, 0)], ('awgn', 1.6, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
        'minsum': ([(0.38, 0), (0.62, 0), (0.78, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
    },
    '11n_1/2_z27': {
        'sumprod2': ([(0.34, 0), (0.7, 0), (0.86, 0)], ('awgn', 1.6, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
        'minsum': ([(0.34, 0), (0.7, 0), (0.82, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
    },
    '16_5/6_z24': {
        'sumprod2': ([(0.34, 0), (0.5, 0), (0.54, 2)], (0.12, 0), (3.0, 0), (0.6, 0), 2, (0.6, 0)),
        'minsum': ([(0.34, 0), (0.5, 0), (0.54, 7)], (0.12, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
    },
    'syn_dc8': {
        'sumprod2': ([(0.42, 0), (0.78, 0), (0.9, 1)], (0.12, 1), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
        'minsum': ([(0.42, 0), (0.74, 0), (0.86, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
    },
    'syn_dc32': {
        'sumprod2': ([(0.38, 0), (0.5, 9), (0.54, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 1, (0.6, 0)),
        'minsum': ([(0.38, 0), (0.54, 0), (0.54, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
    },
    '16_1/2_z96': {
        'sumprod2': ([(0.34, 0), (0.54, 0), (0.82, 0)], ('awgn', 1.6, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
        'minsum': ([(0.34, 0), (0.5, 0), (0.74, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0, (0.6, 0)),
    },
    '16_5/6_z192': {
        'sumprod2': ([(0.3, 0), (0.54, 0)], None, None, None, None, None),
        'minsum': ([(0.3, 0), (0.54, 0)], None, None, None, None, None),
    },
    '16_5/6_z300': {
        'sumprod2': ([(0.3, 0), (0.54, 0)], None, None, None, None, None),
        'minsum': ([(0.3, 0), (0.5, 0)], None, None, None, None, None),
    },
    '16_5/6_z864': {
        'sumprod2': ([(0.3, 0), (0.54, 0)], None, None, None, None, None),
        'minsum': ([(0.3, 0), (0.5, 0)], None, None, None, None, None),
    },
}
_KEYS = ("awgn", "hopeless", "gauss", "erase", "sat", "clamp")
SEEDS = {cell: {algo: dict(zip(_KEYS, t)) for algo, t in by.items()} for cell, by in _SEEDS.items()}


def clamp_word(c, sigma, seed):
    """An AWGN word with eight entries at +-DBL_MAX and +-inf, each with the sign of its codeword bit
    (two of either magnitude on zeros and two on ones; all eight on zeros for the synthetic graphs'
    all-zero word): what the joint decoder's saturated LLRs look like, and what the kernel clamps on load."""
    x, ch = lc.awgn_word(c, sigma, seed)
    perm = np.random.RandomState(1000 + seed).permutation(c.N)
    zeros, ones = perm[x[perm] == 0], perm[x[perm] == 1]
    idx = np.concatenate([zeros[:4], ones[:4]]) if len(ones) >= 4 else zeros[:8]
    ch[idx] = (1.0 - 2 * x[idx]) * np.where(np.arange(8) % 2, np.inf, DBL_MAX)
    return ch


def never_converging_word(c, par):
    if par[0] == "awgn":
        return lc.awgn_word(c, par[1], par[2])[1]
    return lc.hopeless_word(c, *par)


def build_words(c, s, two):
    """(labels, CH (W, N)) from one (cell, algorithm) entry of SEEDS."""
    labels, rows = [], []
    if not two:
        x = lc._codeword(c, np.random.RandomState(100))
        labels.append("noiseless")  # stops after 0 sweeps
        rows.append(10.0 * (0.5 - x))
    for sigma, seed in s["awgn"]:
        labels.append("awgn")
        rows.append(lc.awgn_word(c, sigma, seed)[1])
    if two:
        return labels, np.array(rows)
    labels.append("hopeless")
    rows.append(never_converging_word(c, s["hopeless"]))
    labels.append("gauss")
    scale, seed = s["gauss"]
    rows.append(scale * np.random.RandomState(seed).randn(c.N))
    labels += ["erase", "sat", "clamp"]
    rows += [lc.erase_word(c, *s["erase"]), lc.sat_word(c, s["sat"]), clamp_word(c, *s["clamp"])]
    return labels, np.array(rows)


def words(cell, algo, c=None):
    c = c or make_code(cell)
    return build_words(c, SEEDS[cell][algo], cell in TWO_WORDS)


def trace(c, ch, algo, layers=None, rounded=False):
    """(it, apps, margins) of the reference run to K_TRACE."""
    _, it, apps, margins = fr.decode_code(c, ch, algo, max_it=K_TRACE, trace=True, layers=layers, rounded=rounded)
    return it, apps, margins


def movement(apps, apps1):
    """Largest |apps - apps1| relative to max(1, |apps|); two traces of the same length."""
    return llc.perturbation(apps, apps1)


def stop_margins(layers, apps, margins):
    """Per stop test of a trace: the largest threshold at which its decision is safe, i.e. the
    larger of the smallest non-zero |app| and, over the checks of odd parity, the smallest |app| of
    a check's variables (0 where no check is odd)."""
    out = []
    for app, m in zip(apps, margins):
        neg = (app < 0)[layers.var_of].astype(np.int64)
        odd = np.add.reduceat(neg, layers.cstart[:-1]) & 1
        with np.errstate(invalid="ignore"):
            mag = np.where(np.isnan(app), 0.0, np.abs(app))[layers.var_of]
        amin = np.minimum.reduceat(mag, layers.cstart[:-1])
        out.append(max(float(m), float(amin[odd == 1].max()) if odd.any() else 0.0))
    return np.array(out)


def conditioning(c, ch, layers=None):
    """A sumprod2 word's (it, margins, it of the correctly rounded run, movement between the two runs;
    inf when they stop after different sweeps)."""
    it, apps, margins = trace(c, ch, "sumprod2", layers)
    it1, apps1, _ = trace(c, ch, "sumprod2", layers, rounded=True)
    return it, margins, it1, (movement(apps, apps1) if it1 == it else np.inf)


class Ref:
    """The reference's traced decodes of a cell's words, run once to K_TRACE."""

    def __init__(self, cell, algo):
        self.cell, self.algo = cell, algo
        self.c = make_code(cell)
        self.layers = lr.Layers(self.c.vdeg, self.c.cdeg, self.c.intrlv, lr.code_layers(self.c))
        self.labels, self.CH = words(cell, algo, self.c)
        runs = [trace(self.c, ch, algo, self.layers) for ch in self.CH]
        self.its = np.array([t[0] for t in runs])
        self.apps = [t[1] for t in runs]
        self.margins = [t[2] for t in runs]

    def at(self, k, idx=None):
        """(app, it) of the words (all, or those at idx) cut at max_iter = k."""
        idx = range(len(self.CH)) if idx is None else idx
        got = [fr.truncated(self.its[i], self.apps[i], k) for i in idx]
        return np.array([g[0] for g in got]), np.array([g[1] for g in got])

    def check_preconditions(self):
        """From the reference alone: words that stop after 0, 1, 3 and >= 6 sweeps and one that runs
        out; for sumprod2 no knife-edge stop decision (MARGIN = 100 B, see there), the correctly
        rounded run stops after the same sweeps, and no word moves between the two runs by more
        than the recorded bounds (its cell's P, and ten times the median)."""
        cell, algo = self.cell, self.algo
        if algo == "sumprod2":
            assert 0 < P_CELL[cell] <= P <= 10 * P_MEDIAN and B == 16 * P and MARGIN == 100 * B
            for lab, ch, it, tm, apps in zip(self.labels, self.CH, self.its, self.margins, self.apps):
                assert np.all(stop_margins(self.layers, apps[:len(tm)], tm) >= MARGIN), (lab, tm)
                it1, apps1, _ = trace(self.c, ch, algo, self.layers, rounded=True)
                assert it1 == it, (lab, it, it1)
                moved = movement(apps, apps1)
                assert moved <= P_RECHECK * min(P_CELL[cell], 10 * P_MEDIAN), (lab, moved)
        if cell in TWO_WORDS:
            assert 1 <= self.its.min() <= 3 and 4 <= self.its.max() < K_TRACE, self.its
            return
        by = dict(zip(self.labels, self.its))
        assert by["noiseless"] == 0 and by["hopeless"] == K_TRACE, by
        awgn = sorted(it for lab, it in zip(self.labels, self.its) if lab == "awgn")
        assert awgn[0] == 1 and awgn[1] == 3 and 6 <= awgn[2] < K_TRACE, awgn
        assert by["erase"] > 0  # an erased bit leaves its checks unsatisfied
        clamp = self.CH[self.labels.index("clamp")]
        assert np.isposinf(clamp).any() and np.isneginf(clamp).any() or self.c.standard == "synthetic"
        assert (np.abs(clamp) == DBL_MAX).sum() == 4 and np.isinf(clamp).sum() == 4


@functools.lru_cache(maxsize=None)
def reference(cell, algo):
    return Ref(cell, algo)
