"""Shared inputs of the LDPC belief-propagation tests (no tests here): the
cells of DESIGN.md §10's instance table with their seeded words and traced
oracle references, the synthetic protographs that reach the kernel instances
no standard code reaches, and the Lxor point set.  Test infrastructure only:
the product never imports this module."""
import functools

import numpy as np

from oracle import ldpc_oracle as lo

KS = (1, 2, 3, 4, 8, 9, 10, 12)  # truncation points: around the tail hand-offs 1, 3 and 8
K_TRACE = 12
MARGIN = 1e-6  # smallest stop margin a traced word may have: no knife-edge stop decisions
HANDOFFS = (1, 3, 8)


# ---- synthetic protographs ---------------------------------------------------------

def synthetic_proto(row_weights, ncols, z, heavy=None, seed=0):
    """A seeded base matrix (-1: no block, else a shift in [0, z)) whose row r
    has row_weights[r] blocks and whose every column is used; heavy =
    (column, weight) gives that column exactly `weight` blocks."""
    rs = np.random.RandomState(seed)
    nrows = len(row_weights)
    assert max(row_weights) <= ncols and sum(row_weights) >= ncols
    on = np.zeros((nrows, ncols), dtype=bool)
    room = np.array(row_weights, dtype=np.int64)
    free = np.ones(ncols, dtype=bool)  # columns rows may still draw from
    if heavy is not None:
        col, w = heavy
        rows = rs.permutation(nrows)[:w]
        assert len(rows) == w and (room[rows] > 0).all()
        on[rows, col] = True
        room[rows] -= 1
        free[col] = False
    # every remaining column once, into the row with the most room left
    for col in rs.permutation(np.nonzero(~on.any(0))[0]):
        r = int(np.argmax(room - on[:, col] * (ncols + 1)))
        assert room[r] > 0
        on[r, col] = True
        room[r] -= 1
    for r in range(nrows):
        cand = np.nonzero(free & ~on[r])[0]
        assert len(cand) >= room[r]
        # the columns with the fewest blocks so far first (ties at random): no variable of degree 1
        cand = cand[np.argsort(on[:, cand].sum(0) + rs.random_sample(len(cand)), kind="stable")]
        on[r, cand[:room[r]]] = True
    proto = np.where(on, rs.randint(0, z, on.shape), -1).astype(np.int64)
    assert np.array_equal((proto != -1).sum(1), row_weights) and (proto != -1).any(0).all()
    if heavy is not None:
        assert (proto[:, heavy[0]] != -1).sum() == heavy[1]
    return proto


@functools.lru_cache(maxsize=None)
def _synth_class():
    from sparc_ldpc_amd import ldpc

    class SynthCode(ldpc.code):
        """ldpc.code on a given base matrix (code.__init__ calls assign_proto).
        The matrix has no dual-diagonal part: nothing encodes, the words are
        noisy copies of the all-zero codeword."""

        def __init__(self, proto, z, device=None):
            self._given = np.asarray(proto, dtype=np.int64)
            super().__init__("synthetic", "-", z, "A", device)

        def assign_proto(self):
            return self._given

    return SynthCode


# name -> (row weights, columns, heavy column or None, seed); z = 8
SYNTH = {
    "dc8": ((8, 8, 7, 6, 3, 2, 8, 5), 16, None, 1),  # DCMAX=8 full, with checks of degree 2 and 3
    "dc9": ((9, 9, 8, 5, 4, 7, 6, 3), 17, None, 2),  # the first degree of DCMAX=16
    "dc16": ((16, 16, 15, 12, 9, 16), 24, None, 3),  # DCMAX=16 full
    "dc17": ((17, 16, 16, 13, 10, 17), 25, None, 4),  # the first degree of DCMAX=32
    "dc32": ((32, 32, 31, 20, 17), 40, None, 5),  # DCMAX=32 full
    "dv13": ((7,) * 14, 28, (5, 13), 6),  # one column of weight 13: no tail (nq == 0)
}
SYNTH_Z = 8


def synth_proto(name):
    rw, ncols, heavy, seed = SYNTH[name]
    return synthetic_proto(rw, ncols, SYNTH_Z, heavy, seed)


# ---- the cells -----------------------------------------------------------------------
# name -> code, and what lb_info must report for the cell to reach its instance:
# (max_cdeg, max_vdeg, lds_messages, fixed_dc, threads)
CELLS = {
    "16_1/2_z24": (("802.16", "1/2", 24, "A"), (7, 6, 1, 0, 320)),  # DCMAX=8 irregular, tail_var<8>
    "11n_1/2_z27": (("802.11n", "1/2", 27, "A"), (8, 12, 1, 0, 384)),  # DCMAX=8, tail_var<12>
    "16_2/3_z24": (("802.16", "2/3", 24, "A"), (10, 6, 1, 0, 256)),  # DCMAX=16, check-regular, general
    "16_3/4_z24": (("802.16", "3/4", 24, "A"), (15, 4, 1, 0, 256)),  # DCMAX=16 irregular, tail_var<4>
    "11n_5/6_z27": (("802.11n", "5/6", 27, "A"), (22, 4, 1, 0, 256)),  # DCMAX=32 general
    "16_5/6_z24": (("802.16", "5/6", 24, "A"), (20, 4, 1, 20, 256)),  # DCFIX=20, lane-pair tail
    "16_5/6_z48": (("802.16", "5/6", 48, "A"), (20, 4, 1, 20, 256)),
    "16_1/2_z96": (("802.16", "1/2", 96, "A"), (7, 6, 1, 0, 1024)),  # Nc = 1152 > 1024: strided checks
    "16_5/6_z300": (("802.16", "5/6", 300, "A"), (20, 4, 0, 0, 1024)),  # messages in HBM, general DCMAX=32
    "syn_dc8": ("dc8", (8, None, 1, 0, 256)),
    "syn_dc9": ("dc9", (9, None, 1, 0, 256)),
    "syn_dc16": ("dc16", (16, None, 1, 0, 256)),
    "syn_dc17": ("dc17", (17, None, 1, 0, 256)),
    "syn_dc32": ("dc32", (32, None, 1, 0, 256)),
    "syn_dv13": ("dv13", (7, 13, 1, 0, 256)),
}
TWO_WORDS = ("16_5/6_z300",)  # 0.3 s of oracle per word: two AWGN words, one on each side of the tail
ALGOS = ("sumprod2", "sumprod", "minsum")


def make_code(cell, device=None):
    spec = CELLS[cell][0]
    if isinstance(spec, str):
        return _synth_class()(synth_proto(spec), SYNTH_Z, device)
    from sparc_ldpc_amd import ldpc
    return ldpc.code(*spec, device=device)


def _codeword(c, rs):
    if c.standard == "synthetic":
        return np.zeros(c.N, dtype=np.int64)
    return c.encode(rs.randint(0, 2, c.K))


def awgn_word(c, sigma, seed):
    """(x, ch): a codeword through BPSK + AWGN, LLR = 2 y / sigma^2."""
    rs = np.random.RandomState(seed)
    x = _codeword(c, rs)
    return x, 2.0 * ((1 - 2 * x) + sigma * rs.randn(c.N)) / sigma ** 2


def hopeless_word(c, frac, seed):
    """A codeword at confident magnitudes |N(5, 1)| with a share `frac` of its signs wrong: too many
    for any decoder, and no LLR so close to zero that a check's aggregate (a product of up to 32
    tanh) comes near the stop test's zero."""
    rs = np.random.RandomState(seed)
    x = _codeword(c, rs)
    ch = (1.0 - 2 * x) * np.abs(5.0 + rs.randn(c.N))
    ch[rs.random_sample(c.N) < frac] *= -1.0
    return ch


def erase_word(c, sigma, seed):
    """An AWGN word with z consecutive erased bits at +0.0 and another z at -0.0."""
    ch = awgn_word(c, sigma, seed)[1]
    ch[c.z:2 * c.z] = 0.0
    ch[c.N - 2 * c.z:c.N - c.z] = -0.0
    return ch


def sat_word(c, seed):
    """A codeword at |ch| in {40, 800} (1 + exp(-x) rounds to 1, exp underflows) with a few wrong signs."""
    rs = np.random.RandomState(seed)
    x = _codeword(c, rs)
    ch = (1.0 - 2 * x) * np.where(rs.randint(0, 2, c.N), 40.0, 800.0)
    ch[rs.permutation(c.N)[:3]] *= -1.0
    return ch


# Seeds chosen on the CPU from the oracle alone (scripts/ldpc_case_seeds.py) so
# that every precondition the tests assert holds: per (cell, algorithm)
#   "awgn": (sigma, seed) of the words the oracle stops at iterations 1, 3 and 8
#           (TWO_WORDS cells: one word stopping inside 2..7, one inside 9..11),
#   "hopeless": (share of wrong signs, seed), "gauss": (scale, seed), "erase": (sigma, seed), "sat": seed.
_SEEDS = {  # (awgn, hopeless, gauss, erase, sat)
    '16_1/2_z24': {
        'sumprod2': ([(0.3, 2), (0.54, 1), (0.7, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'sumprod': ([(0.3, 2), (0.54, 1), (0.7, 0)], (0.12, 0), (3.0, 0), None, None),
        'minsum': ([(0.3, 2), (0.46, 0), (0.62, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '11n_1/2_z27': {
        'sumprod2': ([(0.34, 0), (0.54, 0), (0.74, 0)], (0.12, 0), (3.0, 1), (0.6, 0), 4),
        'sumprod': ([(0.34, 0), (0.54, 0), (0.74, 0)], (0.12, 0), (3.0, 1), None, None),
        'minsum': ([(0.34, 0), (0.5, 0), (0.66, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_2/3_z24': {
        'sumprod2': ([(0.38, 0), (0.54, 0), (0.66, 0)], (0.12, 0), (3.0, 29), (0.6, 0), 0),
        'sumprod': ([(0.38, 0), (0.54, 0), (0.66, 0)], (0.12, 0), (3.0, 29), None, None),
        'minsum': ([(0.38, 0), (0.54, 0), (0.66, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_3/4_z24': {
        'sumprod2': ([(0.34, 0), (0.46, 0), (0.58, 0)], (0.12, 0), (6.0, 0), (0.6, 1), 0),
        'sumprod': ([(0.34, 0), (0.46, 0), (0.58, 0)], (0.12, 0), (6.0, 0), None, None),
        'minsum': ([(0.34, 0), (0.46, 0), (0.62, 5)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '11n_5/6_z27': {
        'sumprod2': ([(0.34, 0), (0.46, 0), (0.5, 18)], (0.12, 0), (6.0, 1), (0.6, 6), 0),
        'sumprod': ([(0.34, 0), (0.46, 0), (0.5, 18)], (0.12, 0), (6.0, 1), None, None),
        'minsum': ([(0.34, 0), (0.46, 0), (0.54, 2)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_5/6_z24': {
        'sumprod2': ([(0.34, 0), (0.46, 0), (0.46, 1)], (0.12, 0), (6.0, 1), (0.6, 16), 0),
        'sumprod': ([(0.34, 0), (0.46, 0), (0.46, 1)], (0.12, 0), (6.0, 1), None, None),
        'minsum': ([(0.34, 0), (0.46, 0), (0.58, 10)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_5/6_z48': {
        'sumprod2': ([(0.34, 0), (0.42, 0), (0.54, 5)], (0.12, 1), (10.0, 0), (0.5, 0), 0),
        'sumprod': ([(0.34, 0), (0.42, 0), (0.54, 5)], (0.12, 1), (10.0, 0), None, None),
        'minsum': ([(0.34, 0), (0.42, 1), (0.5, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_1/2_z96': {
        'sumprod2': ([(0.34, 0), (0.42, 0), (0.7, 0)], (0.12, 0), (6.0, 1), (0.6, 0), 5),
        'sumprod': ([(0.34, 0), (0.54, 1), (0.7, 0)], (0.12, 0), (6.0, 1), None, None),
        'minsum': ([(0.34, 0), (0.5, 1), (0.7, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    '16_5/6_z300': {
        'sumprod2': ([(0.38, 0), (0.5, 1)], None, None, None, None),
        'sumprod': ([(0.38, 0), (0.54, 19)], None, None, None, None),
        'minsum': ([(0.38, 0), (0.5, 1)], None, None, None, None),
    },
    'syn_dc8': {
        'sumprod2': ([(0.42, 0), (0.58, 0), (0.82, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'sumprod': ([(0.42, 0), (0.58, 0), (0.82, 0)], (0.12, 0), (3.0, 0), None, None),
        'minsum': ([(0.42, 0), (0.58, 0), (0.78, 0)], (0.12, 0), (3.0, 0), (0.6, 1), 0),
    },
    'syn_dc9': {
        'sumprod2': ([(0.42, 0), (0.7, 0), (0.86, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'sumprod': ([(0.42, 0), (0.7, 0), (0.86, 0)], (0.12, 0), (3.0, 0), None, None),
        'minsum': ([(0.42, 0), (0.66, 0), (0.82, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    'syn_dc16': {
        'sumprod2': ([(0.42, 0), (0.54, 0), (0.66, 0)], (0.12, 0), (3.0, 41), (0.6, 0), 0),
        'sumprod': ([(0.42, 0), (0.54, 0), (0.66, 0)], (0.12, 0), (3.0, 41), None, None),
        'minsum': ([(0.42, 0), (0.54, 0), (0.66, 0)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    'syn_dc17': {
        'sumprod2': ([(0.42, 0), (0.58, 0), (0.58, 9)], (0.12, 0), (6.0, 2), (0.6, 0), 0),
        'sumprod': ([(0.42, 0), (0.58, 0), (0.58, 9)], (0.12, 0), (6.0, 2), None, None),
        'minsum': ([(0.42, 0), (0.58, 0), (0.58, 5)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    'syn_dc32': {
        'sumprod2': ([(0.38, 0), (0.46, 0), (0.54, 1)], (0.12, 0), (6.0, 12), (0.6, 6), 0),
        'sumprod': ([(0.38, 0), (0.46, 0), (0.54, 1)], (0.12, 0), (6.0, 12), None, None),
        'minsum': ([(0.38, 0), (0.46, 0), (0.5, 33)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
    'syn_dv13': {
        'sumprod2': ([(0.42, 0), (0.66, 0), (0.86, 1)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
        'sumprod': ([(0.42, 0), (0.66, 0), (0.86, 1)], (0.12, 0), (3.0, 0), None, None),
        'minsum': ([(0.42, 0), (0.66, 0), (0.82, 3)], (0.12, 0), (3.0, 0), (0.6, 0), 0),
    },
}
_KEYS = ("awgn", "hopeless", "gauss", "erase", "sat")
SEEDS = {cell: {algo: dict(zip(_KEYS, t)) for algo, t in by.items()} for cell, by in _SEEDS.items()}


def words(cell, algo, c=None):
    """The cell's words for one algorithm: (labels, CH (W, N))."""
    c = c or make_code(cell)
    s = SEEDS[cell][algo]
    labels, rows = [], []
    if cell not in TWO_WORDS:
        x = _codeword(c, np.random.RandomState(100))
        labels.append("noiseless")
        rows.append(10.0 * (0.5 - x))  # +-5, test_ldpc.py:51-56
    for sigma, seed in s["awgn"]:
        labels.append("awgn")
        rows.append(awgn_word(c, sigma, seed)[1])
    if cell in TWO_WORDS:
        return labels, np.array(rows)
    labels.append("hopeless")
    rows.append(hopeless_word(c, *s["hopeless"]))
    labels.append("gauss")  # i.i.d. LLRs that belong to no codeword
    scale, seed = s["gauss"]
    rows.append(scale * np.random.RandomState(seed).randn(c.N))
    if algo != "sumprod":  # sumprod on erasures or saturated inputs is 0/0 in the reference too
        labels += ["erase", "sat"]
        rows += [erase_word(c, *s["erase"]), sat_word(c, s["sat"])]
    return labels, np.array(rows)


class Ref:
    """The oracle's traced decodes of a cell's words, run once to K_TRACE."""

    def __init__(self, cell, algo):
        self.c = make_code(cell)
        self.labels, self.CH = words(cell, algo, self.c)
        self.its, self.apps, self.margins = [], [], []
        for ch in self.CH:
            _, it, ta, tm = lo._decode(ch, self.c.vdeg, self.c.cdeg, self.c.intrlv, algo, max_it=K_TRACE, trace=True)
            self.its.append(it)
            self.apps.append(ta)
            self.margins.append(tm)
        self.its = np.array(self.its)

    def at(self, k, idx=None):
        """(app, it) of the words (all, or those at idx) cut at max_iter = k."""
        idx = range(len(self.CH)) if idx is None else idx
        got = [lo.truncated(self.CH[i], self.its[i], self.apps[i], k) for i in idx]
        return np.array([g[0] for g in got]), np.array([g[1] for g in got])

    def check_preconditions(self, cell, algo):
        """From the oracle alone: no knife-edge stop decision, finite sumprod,
        words on every side of every hand-off."""
        for lab, tm, ta in zip(self.labels, self.margins, self.apps):
            if lab == "erase":
                # a check that sees an erased bit has the aggregate Lxor(a, +-0) = +-0 + t - t with
                # the same t twice: exactly zero under any exp / log, unsatisfied on both sides
                assert np.all((tm > MARGIN) | (tm == 0.0)), (lab, tm)
            else:
                assert np.all(tm > MARGIN), (lab, tm)
            if algo == "sumprod":
                assert np.isfinite(ta).all(), lab
        if cell in TWO_WORDS:
            assert 2 <= self.its.min() <= 7 and 9 <= self.its.max() <= 11, self.its
            return
        for h in HANDOFFS:  # words that stop before, at and after every hand-off
            assert (self.its < h).any() and (self.its == h).any() and (self.its > h).any(), (h, self.its)
        assert (self.its == K_TRACE).any()  # and a word that runs out


@functools.lru_cache(maxsize=None)
def reference(cell, algo):
    return Ref(cell, algo)


# ---- Lxor points ----------------------------------------------------------------------
LN_SW = 0.881373587019543  # -ln(sqrt(2) - 1): 1 + exp(-x) crosses sqrt(2), log12's branch switch


def lxor_points():
    """(a, b) pairs for Lxor: about 1500, with every edge of exp, log12 and the sign rule."""
    rs = np.random.RandomState(77)
    A, B = [], []
    for scale in (1.0, 6.0, 40.0, 800.0):
        A.append(rs.randn(150) * scale)
        B.append(rs.randn(150) * scale)
    a = np.concatenate([rs.randn(20) * s for s in (1.0, 6.0, 40.0, 800.0)])
    A += [a, a]
    B += [a, -a]  # b = a, b = -a
    # |a + b| and |a - b| within +-1e-6 of the branch switch and on it
    for t in np.concatenate([[LN_SW], LN_SW + rs.uniform(-1e-6, 1e-6, 12), np.nextafter(LN_SW, [0.0, 2.0])]):
        for a0 in (0.1, -0.3, 2.5, -7.0, 30.0):
            for sg in (1.0, -1.0):
                A += [[a0], [a0]]
                B += [[sg * t - a0], [a0 - sg * t]]  # a + b = sg t;  a - b = sg t
    # where 1 + exp(-x) rounds to 1 (x >~ 36.7) and where exp underflows (x >~ 745)
    for t in (36.0, 37.0, 40.0, 745.0, 750.0, 36.7, 36.8, 708.0, 709.8, 744.5):
        for a0 in (0.25, -1.5, 12.0, -20.0, 400.0):
            for sg in (1.0, -1.0):
                A += [[a0], [a0]]
                B += [[sg * t - a0], [a0 - sg * t]]
    # zeros of either sign, subnormals
    v = np.concatenate([rs.randn(12) * 3, [0.0, -0.0, 5e-324, -5e-324, 1e-310, -3e-309, 2.2250738585072014e-308]])
    for z0 in (0.0, -0.0, 5e-324, -1e-310, 2e-308):
        A += [np.full(len(v), z0), v]
        B += [v, np.full(len(v), z0)]
    return np.concatenate([np.ravel(x) for x in A]).astype(np.float64), \
        np.concatenate([np.ravel(x) for x in B]).astype(np.float64)


def lxor_bar(a, b):
    """4 * 2^-52 * max(1, min(|a|, |b|)): each correction term lies in [0, ln 2] and carries at most
    half an ulp of u in [1, 2], one ulp of exp and one of log12 (<= 1.5 * 2^-52); the two final
    additions round once each, in units of the result's size <= max(1, min(|a|, |b|))."""
    return 4 * 2.0 ** -52 * np.maximum(1.0, np.minimum(np.abs(a), np.abs(b)))
