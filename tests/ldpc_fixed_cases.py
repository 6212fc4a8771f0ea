"""Shared inputs of the fixed-point layered min-sum tests (no tests here): the
cells, widths and correction factors, their words (the layered tests' own, plus
the binary32 tests' clamp word) and the NumPy statement's traced decodes
(tests/ldpc_fixed_ref.py).  Test infrastructure only: the product never imports
this module."""
import functools

import numpy as np

import ldpc_cases as lc
import ldpc_f32_cases as fc
import ldpc_fixed_ref as qr
import ldpc_layered_cases as llc

KS = (0, 1, 2, 3, 4, 6, 12)  # max_iter of the truncated decodes
K_TRACE = 12
WIDTHS = ((2, 6, 8), (0, 2, 2), (1, 4, 6), (3, 8, 16))  # (frac_bits, msg_bits, app_bits)
CORRS = (0.75, 1.0, 0.7)  # alpha 12, 16 and 11 (11.2 rounded: the rounding of corr_factor is the statement's)
PIN_WIDTHS = (2, 8, 16)  # wide enough that no clip fires on the pin words: the statement is binary64 min-sum there
PIN_SWEEPS = 6

# name -> (threads per workgroup, lanes per check) the library plans by default:
#   lanes: the largest power of two <= min(largest check degree, 16) with z * lanes <= 768;
#   threads: z * lanes rounded up to 64, and 1024 from 704 on (over a third of a CU's 2048 threads)
CELLS = {
    "16_1/2_z24": (128, 4),  # irregular dc 6/7
    "11n_1/2_z27": (256, 8),  # dv up to 12; z not a multiple of anything useful
    "16_5/6_z24": (384, 16),  # dc 20
    "syn_dc8": (64, 8),  # checks of degree 2 and 3: fewer edges than lanes in a group
    "syn_dc32": (128, 16),
    "16_1/2_z96": (384, 4),
    "16_5/6_z192": (1024, 4),  # the 24 576-byte image
    "16_5/6_z864": (1024, 1),  # the 110 592-byte image: one workgroup a CU
}
SMALL = tuple(CELLS)[:6]
make_code = llc.make_code

# sim_ldpc_mc on 802.16 1/2 z=24, blocks 0..63: the layered tests' sigma
SIM_SIGMA = llc.SIM_SIGMA


# AWGN words (sigma, seed) added where the layered tests' words leave a stopping class empty under the
# fixed-point statement at the default widths (chosen by scripts/ldpc_fixed_case_seeds.py, from the
# statement alone)
EXTRA_AWGN = {
    'syn_dc32': [(0.5, 1)],
    '16_5/6_z864': [(0.54, 0)],
}


def lds_bytes(c):
    """2 Nv + Nmsg, rounded up to 16 as the kernel's launch rounds it."""
    return (2 * c.Nv + c.Nmsg + 15) // 16 * 16


def words(cell, c=None, extra=True):
    """The cell's words: (labels, CH (W, N)).  The layered tests' min-sum words
    (noiseless, AWGN, hopeless, gauss, erase, sat) and the binary32 tests' clamp
    word (+-DBL_MAX and +-inf); the two-word cells get a noiseless and a
    hopeless word of their own, and EXTRA_AWGN's words come last, so that every
    cell holds every stopping class."""
    c = c or make_code(cell)
    labels, CH = llc.words(cell, "minsum", c)
    labels, rows = list(labels), list(CH)
    if cell in llc.TWO_WORDS:
        x = lc._codeword(c, np.random.RandomState(100))
        labels += ["noiseless", "hopeless"]
        rows += [10.0 * (0.5 - x), lc.hopeless_word(c, 0.12, 0)]
    labels.append("clamp")
    rows.append(fc.clamp_word(c, 0.6, 0))
    for sigma, seed in (EXTRA_AWGN.get(cell, ()) if extra else ()):
        labels.append("awgn+")
        rows.append(lc.awgn_word(c, sigma, seed)[1])
    return labels, np.array(rows)


def pin_words(cell, c=None):
    """LLRs that are multiples of 2^-2 in [-3, 3] (no -0.0): the cell's AWGN words and a word of
    no codeword (3 randn, which never converges), halved (at full scale a converging word's |app| passes
    (3, 8, 16)'s rmax = 127 eighths within six sweeps), rounded and clipped."""
    c = c or make_code(cell)
    rows = [ch for lab, ch in zip(*llc.words(cell, "minsum", c)) if lab == "awgn"]
    rows.append(3.0 * np.random.RandomState(0).randn(c.N))
    return np.clip(np.rint(np.array(rows) * 2.0) / 4.0, -3.0, 3.0) + 0.0


class Ref:
    """The statement's traced decodes of a cell's words at one (widths, corr_factor), run once to K_TRACE."""

    def __init__(self, cell, widths, corr):
        self.c = make_code(cell)
        self.layers = layers(cell)
        self.labels, self.CH = words(cell, self.c)
        self.CH.setflags(write=False)
        self.clips = {}
        runs = [qr.decode(ch, None, None, None, None, *widths, corr_factor=corr, max_it=K_TRACE, trace=True,
                          layers=self.layers, clips=self.clips) for ch in self.CH]
        self.its = np.array([t[1] for t in runs])
        self.apps = [t[2] for t in runs]

    def at(self, k, idx=None):
        """(app, it) of the words (all, or those at idx) cut at max_iter = k; k = 0: the channel itself."""
        idx = range(len(self.CH)) if idx is None else idx
        if k == 0:
            return self.CH[list(idx)], np.zeros(len(idx), dtype=np.int64)
        got = [qr.truncated(self.its[i], self.apps[i], k) for i in idx]
        return np.array([g[0] for g in got]), np.array([g[1] for g in got])


@functools.lru_cache(maxsize=None)
def layers(cell):
    c = make_code(cell)
    return qr.Layers(c.vdeg, c.cdeg, c.intrlv, qr.code_layers(c))


@functools.lru_cache(maxsize=None)
def reference(cell, widths=qr.DEFAULT, corr=0.75):
    return Ref(cell, tuple(widths), corr)


def check_preconditions(cell):
    """From the statement alone.  At the default widths and corr_factor 0.75 the
    cell holds words that stop after 0 sweeps, after 1..3, after 4..11 and one
    that runs out at K_TRACE.  Over the cell's words at (1, 4, 6) the channel
    and the r clip fire, and the q and app clips fire wherever the widths let
    them: |q| <= rmax dv and |q + r| <= rmax (1 + dv) (the channel value and one
    message per check, each at most rmax = 7), so with amax = 31 the q clip
    needs a variable of degree >= 5 and the app clip one of degree >= 4; the
    802.16 5/6 codes and syn_dc32 stop at degree 4, syn_dc8 at 3.  At (0, 2, 2)
    (rmax = amax = 1) the channel, q and app clips fire on every cell."""
    its = reference(cell).its
    assert (its == 0).any() and ((its >= 1) & (its <= 3)).any() and ((its >= 4) & (its < K_TRACE)).any() \
        and (its == K_TRACE).any(), (cell, its)
    clips = reference(cell, (1, 4, 6)).clips
    dv = int(make_code(cell).vdeg.max())
    assert clips["channel"] > 0 and clips["r"] > 0, (cell, clips)
    assert (clips["q"] > 0) == (7 * dv > 31) and (clips["app"] > 0) == (7 * (1 + dv) > 31), (cell, dv, clips)
    narrow = reference(cell, (0, 2, 2)).clips
    assert narrow["channel"] > 0 and narrow["q"] > 0 and narrow["app"] > 0, (cell, narrow)
