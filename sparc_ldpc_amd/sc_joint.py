"""Joint SPARC + LDPC decoding on a spatially coupled design.

``CoupledJointDecoder`` is joint.JointDecoder with ``self.op`` a
sc.CoupledOperator: the ``soft`` and ``hard`` exchanges of
JointDecoder.decode_staged run on it unchanged, every step on the device
(coupled AMP from a β₀: ``sa_sc_run``; the section->bit LLRs, the soft and the
one-hot hand-back on the coupled context's β: ``sa_sc_llr``, ``sa_sc_soft_beta0``,
``sa_sc_hard_indices``, ``sa_sc_stage_onehot``; belief propagation in
``libldpc_bp``).  The LDPC code protects the last ``N / log2 M`` sections, the
reference's convention; ``l0 = 0`` and an ``l0`` inside a column block are both
legal.  ``originalHard`` and ``threshold`` decode the unprotected or undecided
sections on a shortened / masked operator, which a coupled design does not
have: they raise ValueError.  mc_joint accepts the decoder with host and device
draws and never pipelines it.
"""
from __future__ import annotations

import math

from .joint import JointDecoder, joint_options, option_keywords
from .operators import SparcOperator, make_ordering
from .sc import CoupledOperator

__all__ = ["CoupledJointDecoder", "COUPLED_MODES"]

COUPLED_MODES = ("soft", "hard")


class _WithTolerances:
    """A CoupledOperator whose run() decodes with the decoder's stop_tol / freeze_tol."""

    def __init__(self, op, stop_tol, freeze_tol):
        self._op, self._tol = op, dict(stop_tol=float(stop_tol), freeze_tol=float(freeze_tol))

    def __getattr__(self, name):
        return getattr(self._op, name)

    def run(self, B, T, early_stop=True, beta0=False):
        self._op.run(B, T, early_stop=early_stop, beta0=beta0, **self._tol)


class CoupledJointDecoder(JointDecoder):
    """Coupled AMP operator (base matrix W over the Hadamard design of `ordering` / `seed`) + LDPC code, for
    B-codeword batches of the soft and hard joint schemes.  AMP runs in binary64 unless told otherwise, as
    joint.joint_decoder's; stop_tol / freeze_tol are every AMP call's; joint_options as
    JointDecoder's."""

    pipelined = False  # mc_joint never cuts a coupled batch into concurrent halves

    def __init__(self, L, M, n, W, code, T, precision=None, device=None, seed=0, ordering=None, stop_tol=0.0,
                 freeze_tol=0.0, **options):
        self.options = joint_options(**options)
        self._llr_kw, self._bp_kw = option_keywords(self.options)
        self.L, self.M, self.n, self.T = int(L), int(M), int(n), int(T)
        self.logm = int(round(math.log2(M)))
        self.code = code
        nl = code.N
        assert nl <= L * self.logm, "LDPC code longer than the SPARC message"
        assert nl % self.logm == 0, "LDPC code must cover whole sections"
        self.ns = nl // self.logm
        self.l0 = self.L - self.ns
        if ordering is None:
            ordering = make_ordering(L, M, n, seed)
        self.parent = SparcOperator(L, M, n, ordering, "hadamard", precision or "fp64", device)
        self.coupled = CoupledOperator(self.parent, W)
        self.stop_tol, self.freeze_tol = float(stop_tol), float(freeze_tol)
        tol = self.stop_tol != 0.0 or self.freeze_tol != 0.0
        self.op = _WithTolerances(self.coupled, stop_tol, freeze_tol) if tol else self.coupled
        self.sub = None
        self._pipeline = None
        self.total_bits = self.L * self.logm
        self.R = (self.L * self.logm - (code.N - code.K)) / n
        self._masked = None
        self._after_first_amp = None
        self._noise = None
        self.last_draw_ms = 0.0

    @staticmethod
    def _check_mode(mode):
        if mode in ("originalHard", "threshold"):
            raise ValueError(f'mode "{mode}" needs a shortened / masked coupled operator, which a coupled design does '
                             f"not have; a CoupledJointDecoder runs {COUPLED_MODES}")
        if mode not in COUPLED_MODES:
            raise ValueError(f"mode must be one of {COUPLED_MODES}")

    def run(self, idx, noise, Pl, mode="soft", soft_iter=2, threshold=0.5, unit_cancel=False):
        self._check_mode(mode)
        return super().run(idx, noise, Pl, mode, soft_iter, threshold, unit_cancel)

    def decode_staged(self, idx, Pl, mode="soft", soft_iter=2, threshold=0.5, unit_cancel=False):
        self._check_mode(mode)
        return super().decode_staged(idx, Pl, mode, soft_iter, threshold, unit_cancel)
