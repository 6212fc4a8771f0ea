"""Shared inputs of the layered belief-propagation tests (no tests here): the
cells of DESIGN.md §10's layered instance table, their seeded words and the
NumPy reference's traced decodes (tests/ldpc_layered_ref.py).  Test
infrastructure only: the product never imports this module."""
import functools

import numpy as np

import ldpc_cases as lc
import ldpc_layered_ref as lr

KS = (1, 2, 3, 4, 6, 12)  # max_iter of the truncated decodes
K_TRACE = 12
ALGOS = lr.ALGOS
# how far the log -> log1p perturbation of Lxor (an ulp per Lxor, what separates the device's
# log from the C library's) may move a sumprod2 word's app through K_TRACE sweeps, relative to
# max(1, |app|): two orders under the tests' bar, so that a word's own conditioning does not
# decide a comparison (a never-converging word can amplify an ulp to 1e-9 within 12 sweeps)
PERTURB = 1e-11

# name -> (code, what layer_info must report: (lds_messages, max_layer, threads))
#   lds_messages 2: r and app in LDS, 1: app in LDS and r in HBM, 0: both in HBM
CELLS = {
    "16_1/2_z24": (None, (2, 24, 192)),  # irregular dc 6/7 (168 edges a layer), DCMAX=8
    "11n_1/2_z27": (None, (2, 27, 256)),  # dv up to 12
    "16_5/6_z24": (None, (2, 24, 512)),  # DCFIX=20
    "syn_dc8": (None, (2, 8, 128)),  # checks of degree 2 and 3
    "syn_dc32": (None, (2, 8, 256)),  # DCMAX=32
    "16_1/2_z96": (None, (2, 96, 704)),  # 672 edges a layer; test_thread_counts: strided over 128 threads
    "16_5/6_z192": (("802.16", "5/6", 192, "A"), (2, 192, 768)),  # the 156 KB LDS image; 3840 edges a layer strided
    "16_5/6_z300": (None, (1, 300, 768)),  # r in HBM
    "16_5/6_z864": (("802.16", "5/6", 864, "A"), (0, 864, 768)),  # app in HBM too; checks strided over 768 threads
}
TWO_WORDS = ("16_5/6_z192", "16_5/6_z300", "16_5/6_z864")  # two AWGN words: the oracle side stays cheap


def make_code(cell, device=None):
    spec = CELLS[cell][0]
    if spec is None:
        return lc.make_code(cell, device)
    from sparc_ldpc_amd import ldpc
    return ldpc.code(*spec, device=device)


# Seeds chosen on the CPU from the NumPy reference alone
# (scripts/ldpc_layered_case_seeds.py) so that every precondition the tests
# assert holds: per (cell, algorithm)
#   "awgn": (sigma, seed) of the words the reference stops after 1, after 3 and after >= 6 sweeps
#           (TWO_WORDS cells: one word stopping after 1..3 sweeps, one after >= 4),
#   "hopeless": (share of wrong signs, seed), "gauss": (scale, seed), "erase": (sigma, seed), "sat": seed.
_SEEDS = {  # (awgn, hopeless, gauss, erase, sat)
    '16_1/2_z24': {
        'sumprod2': ([(0.38, 0), (0.62, 0), (0.82, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'minsum': ([(0.38, 0), (0.62, 0), (0.78, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '11n_1/2_z27': {
        'sumprod2': ([(0.34, 0), (0.7, 0), (0.86, 0)], (0.08, 6), (3.0, 0), (0.6, 0), 0),
        'minsum': ([(0.34, 0), (0.7, 0), (0.82, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_5/6_z24': {
        'sumprod2': ([(0.34, 0), (0.5, 0), (0.54, 2)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'minsum': ([(0.34, 0), (0.5, 0), (0.54, 7)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    'syn_dc8': {
        'sumprod2': ([(0.42, 0), (0.78, 0), (0.9, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'minsum': ([(0.42, 0), (0.74, 0), (0.86, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    'syn_dc32': {
        'sumprod2': ([(0.38, 0), (0.5, 9), (0.54, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'minsum': ([(0.38, 0), (0.54, 0), (0.54, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_1/2_z96': {
        'sumprod2': ([(0.34, 0), (0.54, 0), (0.82, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'minsum': ([(0.34, 0), (0.5, 0), (0.74, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_5/6_z192': {
        'sumprod2': ([(0.3, 0), (0.54, 0)], None, None, None, None),
        'minsum': ([(0.3, 0), (0.54, 0)], None, None, None, None),
    },
    '16_5/6_z300': {
        'sumprod2': ([(0.3, 0), (0.54, 0)], None, None, None, None),
        'minsum': ([(0.3, 0), (0.5, 0)], None, None, None, None),
    },
    '16_5/6_z864': {
        'sumprod2': ([(0.3, 0), (0.54, 0)], None, None, None, None),
        'minsum': ([(0.3, 0), (0.5, 0)], None, None, None, None),
    },
}
_KEYS = ("awgn", "hopeless", "gauss", "erase", "sat")
SEEDS = {cell: {algo: dict(zip(_KEYS, t)) for algo, t in by.items()} for cell, by in _SEEDS.items()}

# sim_ldpc_mc on 802.16 1/2 z=24, blocks 0..63: the sigma at which, by the
# references alone, the layered decoder leaves no more bit errors than flooding
# (0 and 0; at 0.8: flooding 12, layered 87; at 0.85: 625 and 471)
SIM_SIGMA = 0.75


def words(cell, algo, c=None):
    """The cell's words for one algorithm: (labels, CH (W, N))."""
    c = c or make_code(cell)
    s = SEEDS[cell][algo]
    labels, rows = [], []
    if cell not in TWO_WORDS:
        x = lc._codeword(c, np.random.RandomState(100))
        labels.append("noiseless")  # stops after 0 sweeps
        rows.append(10.0 * (0.5 - x))
    for sigma, seed in s["awgn"]:
        labels.append("awgn")
        rows.append(lc.awgn_word(c, sigma, seed)[1])
    if cell in TWO_WORDS:
        return labels, np.array(rows)
    labels.append("hopeless")
    rows.append(lc.hopeless_word(c, *s["hopeless"]))
    labels.append("gauss")
    scale, seed = s["gauss"]
    rows.append(scale * np.random.RandomState(seed).randn(c.N))
    labels += ["erase", "sat"]
    rows += [lc.erase_word(c, *s["erase"]), lc.sat_word(c, s["sat"])]
    return labels, np.array(rows)


def trace(c, ch, algo, layers=None, log1p=False):
    """(it, apps, margins) of the reference run to K_TRACE."""
    _, it, apps, margins = lr.decode_code(c, ch, algo, max_it=K_TRACE, trace=True, layers=layers, log1p=log1p)
    return it, apps, margins


def acceptable(c, ch, algo, layers=None):
    """No knife-edge stop: every stop test's smallest non-zero |app| is at
    least MARGIN, and the log1p variant of Lxor stops after the same sweeps.
    Returns (ok, it)."""
    it, apps, margins = trace(c, ch, algo, layers)
    ok = bool(np.all(margins >= lc.MARGIN))
    if ok and algo == "sumprod2":
        it1, apps1, _ = trace(c, ch, algo, layers, log1p=True)
        ok = it1 == it and perturbation(apps, apps1) <= PERTURB
    return ok, it


def perturbation(apps, apps1):
    with np.errstate(invalid="ignore"):
        d = np.abs(apps - apps1) / np.maximum(1.0, np.abs(apps))
    return float(np.max(np.where(apps == apps1, 0.0, d)))


class Ref:
    """The reference's traced decodes of a cell's words, run once to K_TRACE."""

    def __init__(self, cell, algo):
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
        got = [lr.truncated(self.its[i], self.apps[i], k) for i in idx]
        return np.array([g[0] for g in got]), np.array([g[1] for g in got])

    def check_preconditions(self, cell, algo):
        """From the reference alone: no knife-edge stop decision, and words
        that stop after 0, 1, 3 and >= 6 sweeps and one that runs out."""
        for lab, ch, it, tm, apps in zip(self.labels, self.CH, self.its, self.margins, self.apps):
            if algo == "sumprod2":
                assert np.all(tm >= lc.MARGIN), (lab, tm)
                it1, apps1, _ = trace(self.c, ch, algo, self.layers, log1p=True)
                assert it1 == it and perturbation(apps, apps1) <= PERTURB, lab
        if cell in TWO_WORDS:
            assert 1 <= self.its.min() <= 3 and 4 <= self.its.max() < K_TRACE, self.its
            return
        by = dict(zip(self.labels, self.its))
        assert by["noiseless"] == 0 and by["hopeless"] == K_TRACE, by
        awgn = sorted(it for lab, it in zip(self.labels, self.its) if lab == "awgn")
        assert awgn[0] == 1 and awgn[1] == 3 and 6 <= awgn[2] < K_TRACE, awgn
        assert by["erase"] > 0  # an erased bit leaves its checks unsatisfied


@functools.lru_cache(maxsize=None)
def reference(cell, algo):
    return Ref(cell, algo)
