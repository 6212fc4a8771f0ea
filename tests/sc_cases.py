"""The case table of the spatially coupled decoder's tests (CPU statement and
GPU): shapes, base matrices, channel, seeds and, where the statement decodes
every section, the stop index it reaches (T = 24, early stop on)."""
import numpy as np

from oracle import amp_oracle as orc
import sc_ref


class Case:
    def __init__(self, name, L, M, n, omega, Lambda, P, sigma, seeds, stops=None, pa=None):
        self.name, self.L, self.M, self.n = name, L, M, n
        self.omega, self.Lambda, self.P, self.sigma = omega, Lambda, P, sigma
        self.seeds = tuple(seeds)
        self.stops = dict(stops or {})  # seed -> stop index of a full decode
        self.W = sc_ref.base_matrix(omega, Lambda)
        self.R, self.C = self.W.shape
        self.Pl = np.full(L, P / L) if pa is None else pa
        self._A = None
        self._ord = None

    @property
    def ordering(self):
        if self._ord is None:
            self._ord = orc.make_ordering(self.L, self.M, self.n, 0)
        return self._ord

    @property
    def A(self):
        """The dense coupled design, built once per process."""
        if self._A is None:
            self._A = sc_ref.coupled_matrix(self.L, self.M, self.n, self.W, self.ordering)
        return self._A

    def rep(self, seed):
        return sc_ref.rep(self.L, self.M, self.n, self.Pl, self.sigma, self.A, seed)


A = Case("A", 32, 64, 160, 2, 4, 2.0, 0.4, (1, 2, 3), {1: 8})  # seeds 2, 3: hard trajectories, parity only
B = Case("B", 24, 512, 256, 2, 3, 4.0, 0.5, (1, 2, 3), {1: 5, 2: 6, 3: 6})
C = Case("C", 15, 16, 185, 3, 3, 3.0, 0.6, (1, 2, 3), {1: 4, 2: 4, 3: 4})
D = Case("D", 48, 32, 300, 3, 8, 2.5, 0.5, (1, 2, 3), {1: 7, 2: 7, 3: 7})
# case A with an exponential power allocation: parity only
E = Case("E", 32, 64, 160, 2, 4, 2.0, 0.4, (1, 2, 3),
         pa=orc.pa_parameterised(32, 0.5 * np.log2(1 + 2.0 / 0.4 ** 2), 2.0, 1.0, 0.5))

CASES = {c.name: c for c in (A, B, C, D, E)}
LAYOUT_CASES = (A, B, C, D)
# (case, seed) the statement decodes completely, with its stop index
DECODED = [(c, s) for c in (A, B, C, D) for s in c.seeds if s in c.stops]
# every trajectory
TRAJ = [(c, s) for c in (A, B, C, D, E) for s in c.seeds]

# the reduction to the uncoupled decoder
FLAT = dict(L=32, M=64, n=192, P=2.0, sigma=0.5, seed=1234, T=12)
FLAT_W = {"1x1": np.ones((1, 1)), "1x4": np.ones((1, 4))}
