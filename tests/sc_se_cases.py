"""Shared inputs of the coupled state-evolution tests (no tests here): the
cases of tests/test_gpu_sc_se.py and tests/test_sc_se_host.py, their Gaussian
rows, and the NumPy statement's results (tests/sc_se_ref.py), computed once per
case.  Test infrastructure only: the product never imports this module."""
import functools

import numpy as np

import sc_ref
import sc_se_ref
from se_cases import MARGIN, MAX_M, TOL_FACTOR, _cap, _pa, rows_of  # noqa: F401  (the project's convention)

MAX_BLOCKS = 64  # SA_SC_MAX_BLOCKS of include/sparc_amp.h

_GENERAL_W = np.array([[1.5, 0.5, 0.0, 0.0, 2.0],
                       [0.0, 1.0, 1.25, 0.75, 0.0],
                       [1.5, 1.5, 1.75, 2.25, 1.0]])  # no band, R < C, every column of mean 1


def _band(omega, Lambda):
    return sc_ref.base_matrix(omega, Lambda)


# name -> (L, M, P, S, T, configurations); a configuration: (n, W, sigma, allocation),
#   an allocation: "uniform", ("distinct",) L distinct powers, or ("pa", a, f)
CASES = {
    # fewer columns than lanes; the uncoupled limit
    "flat_1x1": (8, 4, 2.0, 3, 8, ((16, np.ones((1, 1)), 0.6, "uniform"),)),
    # S no multiple of a chunk; T far past convergence: the skip and the stop index
    "band_2_4": (32, 64, 2.0, 33, 40, ((160, _band(2, 4), 0.4, "uniform"),)),
    # M no power of two; several classes a block; the flat tail's one power in two blocks
    "pa_blocks": (16, 100, 1.8, 33, 8, ((150, _band(3, 4), 0.5, ("pa", 1.0, 0.5)),)),
    # not a band; R < C
    "general_W": (10, 16, 2.0, 5, 6, ((30, _GENERAL_W, 0.5, ("distinct",)),)),
    # every lane a row block: R = 64, C = 61
    "rows_64": (61, 8, 2.0, 2, 3, ((128, _band(4, 61), 0.5, "uniform"),)),
    # every lane both: R = C = 64
    "square_64": (64, 4, 2.0, 2, 3, ((64, _band(1, 64), 0.5, "uniform"),)),
    # R, C, n, sigma and class counts differ inside one call; padding
    "batch_mixed": (24, 32, 2.0, 17, 6, ((100, np.ones((1, 1)), 0.5, "uniform"),
                                         (100, _band(2, 3), 0.6, "uniform"),
                                         (102, _band(3, 4), 0.7, ("distinct",)))),
    # the largest row the kernel holds
    "max_M": (2, MAX_M, 2.0, 2, 2, ((24, _band(2, 2), 0.5, "uniform"),)),
}

# Chosen on the CPU from the statement alone (scripts/sc_se_case_seeds.py --write):
# name -> (base seed: the first from 0 at which every miss comparison of the case
# has a relative margin >= MARGIN and the binary64 and longdouble statements agree
# on every miss count and stop index; the largest binary64-against-longdouble gap
# in phi, tau2, x and E)
# --- chosen: begin ---
_CHOSEN = {
    'flat_1x1': (0, 3.095397202446115e-16),
    'band_2_4': (1, 1.3147035543559227e-15),
    'pa_blocks': (0, 6.285119993898469e-16),
    'general_W': (0, 4.135147085859714e-16),
    'rows_64': (0, 3.850001914496026e-16),
    'square_64': (0, 2.6281060661048627e-16),
    'batch_mixed': (0, 3.1281401080551774e-15),
    'max_M': (0, 1.0274983988645126e-15),
}
# --- chosen: end ---


def allocation(L, P, sigma, kind):
    if kind == "uniform":
        return P / L * np.ones(L)
    if kind[0] == "distinct":
        w = np.arange(L, 0, -1, dtype=np.float64) + 0.37
        return P * w / w.sum()
    return _pa(L, _cap(P, sigma), P, kind[1], kind[2])


def configurations(name):
    """[(n, W, sigma, Pl)] of a case."""
    L, M, P, S, T, cfgs = CASES[name]
    return [(n, np.array(W, dtype=np.float64), float(sg), allocation(L, P, sg, kind)) for n, W, sg, kind in cfgs]


def statement(name, seed, longdouble=False, margin=False):
    """The statement's result of every configuration of a case on the rows of `seed`."""
    L, M, P, S, T, _ = CASES[name]
    U = rows_of(seed, S, M)
    return [sc_se_ref.sc_se_ref(Pl, sg, M, n, W, T, U, longdouble=longdouble, margin=margin)
            for n, W, sg, Pl in configurations(name)]


class Case:
    """A case's inputs and the statement's results, computed once."""

    def __init__(self, name):
        self.name = name
        self.L, self.M, self.P, self.S, self.T, _ = CASES[name]
        cfgs = configurations(name)
        self.B = len(cfgs)
        self.n = [c[0] for c in cfgs]
        self.W = [c[1] for c in cfgs]
        self.sigma = np.array([c[2] for c in cfgs])
        self.Pl = np.array([c[3] for c in cfgs])
        self.R = [w.shape[0] for w in self.W]
        self.C = [w.shape[1] for w in self.W]
        self.seed, self.gap = _CHOSEN[name]
        self.tol = TOL_FACTOR * self.gap
        self.seeds = self.seed + np.arange(self.S)
        self.U = rows_of(self.seed, self.S, self.M)
        ref = [sc_se_ref.sc_se_ref(self.Pl[b], self.sigma[b], self.M, self.n[b], self.W[b], self.T, self.U, margin=True)
               for b in range(self.B)]
        self.phi, self.tau2, self.x, self.miss, self.E, self.stop, margins = (list(v) for v in zip(*ref))
        self.margin = min(margins)
        for a in [self.U, self.Pl, self.sigma] + self.W + self.phi + self.tau2 + self.x + self.miss + self.E:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
