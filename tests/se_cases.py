"""Shared inputs of the state-evolution tests (no tests here): the cases of
tests/test_gpu_se.py, their Gaussian rows, and the NumPy statement's results
(tests/se_ref.py), computed once per case.  Test infrastructure only: the
product never imports this module."""
import functools

import numpy as np

import se_ref

MAX_M = 4096  # SA_SE_MAX_M of include/sparc_amp.h
MARGIN = 1e-9  # least relative margin of every miss comparison (a rounding difference cannot flip a count)
TOL_FACTOR = 64  # tolerance = TOL_FACTOR * the case's binary64-against-longdouble gap, absolute


def _pa(L, C, P, a, f):  # harness.pa_parameterised (sparc_ldpc.py:172-186)
    pa = 2 ** (-2 * a * C * np.arange(L) / L)
    pa[int(f * L):] = pa[int(f * L)]
    pa /= pa.sum() / P
    return pa


def _cap(P, sigma):
    return 0.5 * np.log2(1.0 + P / sigma ** 2)


# name -> (L, M, R, P, sigmas (one per allocation), S, T, allocations)
#   an allocation: "uniform", ("distinct",) five distinct powers, or ("pa", a, f)
CASES = {
    "closed_form": (1, 2, 1.0, 1.0, (0.7,), 1, 1, ("uniform",)),  # one accepted polar pair
    "odd_M": (4, 3, 1.0, 1.0, (0.6,), 2, 4, ("uniform",)),  # the cached Gaussian partner is dropped
    "few_columns": (8, 4, 1.0, 2.0, (0.6,), 3, 8, ("uniform",)),  # fewer columns than lanes; one class x 8
    "distinct": (5, 64, 0.8, 2.0, (0.5,), 257, 8, (("distinct",),)),  # S no multiple of a chunk; every class x 1
    "not_pow2": (16, 100, 0.7, 1.8, (0.5,), 33, 8, (("pa", 1.0, 0.7),)),  # partial last lane pass; flat-tail class
    "batch3": (40, 512, 1.0, 4.0, (1.0, 1.1247, 1.3), 64, 8,
               ("uniform", ("pa", 1.0, 0.7), ("pa", 0.5, 0.3))),  # class counts and sigma differ per allocation
    "max_M": (2, MAX_M, 1.0, 2.0, (0.5,), 2, 2, ("uniform",)),  # the largest row the kernel holds
}

# Chosen on the CPU from the statement alone (scripts/se_case_seeds.py --write):
# name -> (base seed: the first from 0 at which every miss comparison of the case
# has a relative margin >= MARGIN; the largest binary64-against-longdouble gap in
# tau2 and x)
# --- chosen: begin ---
_CHOSEN = {
    'closed_form': (0, 5.702903427273753e-17),
    'odd_M': (0, 9.768661574094395e-17),
    'few_columns': (0, 3.095397202446115e-16),
    'distinct': (0, 5.042624304230081e-16),
    'not_pow2': (0, 4.060879237044457e-16),
    'batch3': (0, 1.2091022627558345e-15),
    'max_M': (0, 8.456776945386935e-18),
}
# --- chosen: end ---


def code_length(name):
    L, M, R = CASES[name][:3]
    return int(L * np.log2(M) / R)


def allocations(name):
    """Pl (B, L) and sigma (B,) of a case."""
    L, M, R, P, sigmas, S, T, allocs = CASES[name]
    rows = []
    for kind, sg in zip(allocs, sigmas):
        if kind == "uniform":
            rows.append(P / L * np.ones(L))
        elif kind[0] == "distinct":
            w = np.arange(L, 0, -1, dtype=np.float64) + 0.37
            rows.append(P * w / w.sum())
        else:
            rows.append(_pa(L, _cap(P, sg), P, kind[1], kind[2]))
    return np.array(rows), np.array(sigmas, dtype=np.float64)


def rows_of(seed, S, M):
    """Row s = RandomState(seed + s).randn(M): what the seeded path draws."""
    return np.array([np.random.RandomState(seed + s).randn(M) for s in range(S)])


def statement(name, seed, longdouble=False, margin=False):
    L, M, R, P, sigmas, S, T, allocs = CASES[name]
    Pl, sig = allocations(name)
    return se_ref.se_ref(Pl, sig, M, code_length(name), T, rows_of(seed, S, M), longdouble=longdouble, margin=margin)


class Case:
    """A case's inputs and the statement's results, computed once."""

    def __init__(self, name):
        self.name = name
        self.L, self.M, self.R, self.P, _, self.S, self.T, _ = CASES[name]
        self.n = code_length(name)
        self.Pl, self.sigma = allocations(name)
        self.B = len(self.Pl)
        self.seed, self.gap = _CHOSEN[name]
        self.tol = TOL_FACTOR * self.gap
        self.seeds = self.seed + np.arange(self.S)
        self.U = rows_of(self.seed, self.S, self.M)
        self.U.setflags(write=False)
        self.tau2, self.x, self.miss, self.E, self.margin = se_ref.se_ref(
            self.Pl, self.sigma, self.M, self.n, self.T, self.U, margin=True)
        for a in (self.tau2, self.x, self.miss, self.E, self.Pl, self.sigma):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
