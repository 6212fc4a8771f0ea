"""Spatially coupled SPARCs: base-matrix AMP on the device (``sa_sc_*`` in
include/sparc_amp.h, kernels ``k_scsec`` / ``k_scrow``).

The coupled design over the sub-sampled Hadamard operator Ã of
``sparc_transforms(L, M, n, seed)`` is ``A[i, j] = sqrt(W[r(i), c(j)]) Ã[i, j]``
for an R x C base matrix W: row i lies in row block ``i // (n // R)``, section l
in column block ``l // (L // C)``.  AMP tracks one effective-noise level per
row block (φ_r) and per column block (τ_c²); at ``W = [[1]]`` it is ``amp()``.

Opt-in (``sa_sc_amp_ex`` / ``sa_sc_mc_ex``): ``stop_tol``
stops a codeword once every φ_r is within ``stop_tol`` (relative) of the
previous iteration's, ``freeze_tol`` leaves a column block alone while its τ_c²
is within ``freeze_tol`` of the value its β was last computed at, and
``return_live`` adds the (B, T, C) uint8 trace of the blocks that were computed.
At the defaults (0, 0, False) every call is what it was.

A decode may start from a β₀ (``beta0`` / ``beta``: β = β₀, z = y − A β₀, then
the same loop; ``sa_sc_amp_start``), and a CoupledOperator has SparcOperator's
device-resident life cycle (reserve, stage_power, stage / encode / encode_bits,
run, wait, decide, fetch_beta) and its SPARC <-> LDPC glue (llr, soft_beta0,
hard_cancel, stage_onehot) on the coupled context's β, which is what
sc_joint.CoupledJointDecoder runs on.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import as_f64, check, dptr
from .operators import SparcOperator, _cached_operator, llr_mode, make_ordering, seed_array

__all__ = ["base_matrix", "CoupledOperator", "ScAbOp", "ScAzOp", "sc_transforms", "amp_sc", "amp_sc_batch",
           "mc_decode_sc"]


def base_matrix(omega: int, Lambda: int) -> np.ndarray:
    """The (ω, Λ) band-diagonal base matrix: R = Λ + ω - 1 rows, C = Λ columns,
    W[r, c] = R / ω for c <= r <= c + ω - 1 and 0 elsewhere.  Every column has
    mean 1, so each column of the coupled design keeps unit average norm."""
    omega, Lambda = int(omega), int(Lambda)
    if omega < 1 or Lambda < 1:
        raise ValueError("omega and Lambda must be at least 1")
    R = Lambda + omega - 1
    W = np.zeros((R, Lambda))
    for c in range(Lambda):
        W[c:c + omega, c] = R / omega
    return W


class CoupledOperator:
    """A coupled design on the device (one ``sa_sc``) over a Hadamard-backend
    SparcOperator, whose tables it borrows and which it keeps alive."""

    def __init__(self, parent: SparcOperator, W):
        lib = _lib.load()
        if not hasattr(lib, "sa_sc_create"):
            raise _lib.SparcAmpError(_lib.SA_ERR_UNSUPPORTED, "this build of the library has no sa_sc_create")
        W = as_f64(W)
        if W.ndim != 2:
            raise ValueError("W must be a 2-d base matrix (R x C)")
        self.parent = parent
        self.W = W
        self.R, self.C = int(W.shape[0]), int(W.shape[1])
        self.L, self.M, self.n = parent.L, parent.M, parent.n
        self.precision, self.device = parent.precision, parent.device
        self._lib = lib
        self._sc = _lib.ct.c_void_p()
        check(lib.sa_sc_create(parent.ctx, self.R, self.C, dptr(W), _lib.ct.byref(self._sc)))

    def __del__(self):
        sc = getattr(self, "_sc", None)
        if sc is not None and sc.value:
            try:
                self._lib.sa_sc_destroy(sc)
            except Exception:
                pass
            self._sc = None

    def Ab_batch(self, beta) -> np.ndarray:
        """A β for a (B, L*M) batch -> (B, n)."""
        beta = as_f64(beta)
        B = beta.shape[0]
        assert beta.size == B * self.L * self.M
        out = np.empty((B, self.n))
        check(self._lib.sa_sc_Ab(self._sc, B, dptr(beta), dptr(out)))
        return out

    def Az_batch(self, z) -> np.ndarray:
        """Aᵀ z for a (B, n) batch -> (B, L*M)."""
        z = as_f64(z)
        B = z.shape[0]
        assert z.size == B * self.n
        out = np.empty((B, self.L * self.M))
        check(self._lib.sa_sc_Az(self._sc, B, dptr(z), dptr(out)))
        return out

    def _ex(self, name, stop_tol, freeze_tol, return_live):
        """The `_ex` entry point where a tolerance or the live trace asks for it, else None."""
        stop_tol, freeze_tol = float(stop_tol), float(freeze_tol)
        if stop_tol == 0.0 and freeze_tol == 0.0 and not return_live:
            return None
        if not hasattr(self._lib, name):
            raise _lib.SparcAmpError(_lib.SA_ERR_UNSUPPORTED, f"this build of the library has no {name}: stop_tol, "
                                     "freeze_tol and return_live need it")
        return getattr(self._lib, name)

    def _need(self, name):
        """A late entry point of the library, or SA_ERR_UNSUPPORTED naming it."""
        if not hasattr(self._lib, name):
            raise _lib.SparcAmpError(_lib.SA_ERR_UNSUPPORTED, f"this build of the library has no {name}")
        return getattr(self._lib, name)

    def amp_batch(self, y, Pl, T, early_stop=True, stop_tol=0.0, freeze_tol=0.0, return_live=False, beta0=None):
        """Decode B codewords: y (B, n) -> (β̂ (B, L*M), iters (B,), φ (B, T, R)).
        beta0 (B, L*M) or None: the start, β = β₀ and z = y − A β₀ (None: β = 0).
        iters[b] is the stop index (every φ_r bit-equal to the previous
        iteration's, or within stop_tol of it), or T; φ rows from the stop
        index on are zero.  return_live appends live (B, T, C) uint8: 1 where
        block c was computed in iteration t (0 from the stop index on)."""
        y = as_f64(y)
        B = y.shape[0] if y.ndim == 2 else 1
        assert y.size == B * self.n, "y must hold B x n values"
        Pl = as_f64(Pl).reshape(-1)
        assert Pl.size == self.L, "Pl must hold L section powers"
        T = int(T)
        assert T >= 0
        out = np.empty((B, self.L * self.M))
        iters = np.empty(B, dtype=np.int32)
        phi = np.zeros((B, T, self.R))
        flags = 0 if early_stop else _lib.SA_FLAG_NO_EARLY_STOP
        ip = iters.ctypes.data_as(_lib.ct.POINTER(_lib.ct.c_int))
        if beta0 is not None:
            beta0 = as_f64(beta0)
            assert beta0.size == B * self.L * self.M, "β₀ must hold L*M values per codeword"
            live = np.zeros((B, T, self.C), dtype=np.uint8) if return_live else None
            lp = live.ctypes.data_as(_lib.ct.POINTER(_lib.ct.c_ubyte)) if return_live else None
            check(self._need("sa_sc_amp_start")(self._sc, B, dptr(y), dptr(Pl), T, dptr(beta0), float(stop_tol),
                                                float(freeze_tol), dptr(out), ip, dptr(phi), lp, flags))
            return (out, iters, phi, live) if return_live else (out, iters, phi)
        ex = self._ex("sa_sc_amp_ex", stop_tol, freeze_tol, return_live)
        if ex is None:
            check(self._lib.sa_sc_amp(self._sc, B, dptr(y), dptr(Pl), T, dptr(out), ip, dptr(phi), flags))
            return out, iters, phi
        live = np.zeros((B, T, self.C), dtype=np.uint8) if return_live else None
        lp = live.ctypes.data_as(_lib.ct.POINTER(_lib.ct.c_ubyte)) if return_live else None
        check(ex(self._sc, B, dptr(y), dptr(Pl), T, float(stop_tol), float(freeze_tol), dptr(out), ip, dptr(phi), lp, flags))
        return (out, iters, phi, live) if return_live else (out, iters, phi)

    def last_amp_ms(self) -> float:
        """Device milliseconds of the last amp_batch's iterations (events)."""
        return float(self._lib.sa_sc_event_ms(self._sc))

    def state_evolution(self, Pl, sigma, T, **kw):
        """Coupled state evolution of this design (its own W, M and n): what
        amp_batch's φ trace and error rate are predicted to be, without a
        codeword.  -> se.SCSEResult; kw goes to se.sc_state_evolution."""
        from .se import sc_state_evolution
        kw.setdefault("device", self.device)
        return sc_state_evolution(Pl, self.M, self.n, self.W, sigma, T, **kw)

    def mc(self, idx, noise, Pl, T, early_stop=True, stop_tol=0.0, freeze_tol=0.0, return_live=False):
        """Encode (y = A β(idx) + noise), decode, decide and count bit errors on
        the device in one call: idx (B, L) int32, noise (B, n) or None ->
        (decisions (B, L), stop indices (B,), bit errors (B,), device ms), and
        with return_live the live trace (B, T, C) uint8 behind them."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        B = idx.shape[0]
        assert idx.shape == (B, self.L), "idx must be (B, L)"
        nz = None
        if noise is not None:
            noise = as_f64(noise)
            assert noise.size == B * self.n, "noise must be (B, n)"
            nz = dptr(noise)
        Pl = as_f64(Pl).reshape(-1)
        assert Pl.size == self.L, "Pl must hold L section powers"
        i32 = _lib.ct.POINTER(_lib.ct.c_int32)
        dec = np.empty((B, self.L), dtype=np.int32)
        its = np.empty(B, dtype=np.int32)
        errs = np.empty(B, dtype=np.int32)
        ms = np.zeros(1)
        flags = 0 if early_stop else _lib.SA_FLAG_NO_EARLY_STOP
        ex = self._ex("sa_sc_mc_ex", stop_tol, freeze_tol, return_live)
        if ex is None:
            check(self._lib.sa_sc_mc(self._sc, B, idx.ctypes.data_as(i32), nz, dptr(Pl), int(T), flags,
                                     dec.ctypes.data_as(i32), its.ctypes.data_as(i32), errs.ctypes.data_as(i32), dptr(ms)))
            return dec, its, errs, float(ms[0])
        live = np.zeros((B, int(T), self.C), dtype=np.uint8) if return_live else None
        lp = live.ctypes.data_as(_lib.ct.POINTER(_lib.ct.c_ubyte)) if return_live else None
        check(ex(self._sc, B, idx.ctypes.data_as(i32), nz, dptr(Pl), int(T), float(stop_tol), float(freeze_tol), flags,
                 dec.ctypes.data_as(i32), its.ctypes.data_as(i32), errs.ctypes.data_as(i32), lp, dptr(ms)))
        return (dec, its, errs, float(ms[0]), live) if return_live else (dec, its, errs, float(ms[0]))


    # ---- the staged, device-resident path (SparcOperator's names and signatures) ----
    _I32 = _lib.ct.POINTER(_lib.ct.c_int32)

    def reserve(self, B, T):
        check(self._need("sa_sc_reserve")(self._sc, int(B), int(T)))

    def stage_power(self, B, Pl):
        """Stage the section powers (c_l = sqrt(n Pl_l)); B is SparcOperator's argument and is not needed here."""
        Pl = as_f64(Pl).reshape(-1)
        assert Pl.size == self.L, "Pl must hold L section powers"
        check(self._need("sa_sc_stage_power")(self._sc, dptr(Pl)))

    def stage(self, y, Pl=None, beta0=None):
        """Stage y (B, n), with Pl the section powers and with beta0 (B, L*M) a start for run(beta0=True)."""
        y = as_f64(y)
        B = y.shape[0] if y.ndim == 2 else 1
        assert y.size == B * self.n, "y must hold B x n values"
        if Pl is not None:
            self.stage_power(B, Pl)
        if beta0 is not None:
            beta0 = as_f64(beta0)
            assert beta0.size == B * self.L * self.M, "β₀ must hold L*M values per codeword"
        check(self._need("sa_sc_stage")(self._sc, B, dptr(y), None if beta0 is None else dptr(beta0)))
        return B

    def encode(self, idx, noise=None):
        """Stage y = A β(idx) + noise; idx (B, L) section indices."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        B = idx.shape[0]
        assert idx.shape == (B, self.L)
        nz = None
        if noise is not None:
            noise = as_f64(noise)
            assert noise.size == B * self.n
            nz = dptr(noise)
        check(self._need("sa_sc_encode")(self._sc, B, idx.ctypes.data_as(self._I32), nz))
        return B

    def encode_bits(self, B, d_bits, d_noise=None, fetch_idx=True):
        """encode from message bits on the device (SparcOperator.encode_bits): int device pointers to (B, L log2 M)
        uint8 bits and to (B, n) float64 noise or None.  Returns the section indices (B, L) int32 (None without
        fetch_idx)."""
        idx = np.empty((int(B), self.L), dtype=np.int32) if fetch_idx else None
        check(self._need("sa_sc_encode_bits")(self._sc, int(B), _lib.ct.c_void_p(d_bits), _lib.ct.c_void_p(d_noise),
                                              None if idx is None else idx.ctypes.data_as(self._I32)))
        return idx

    def run(self, B, T, early_stop=True, beta0=False, stop_tol=0.0, freeze_tol=0.0):
        """Queue a decode of the staged y; beta0: start from the β on the device (staged, soft_beta0's,
        stage_onehot's or the last run's)."""
        flags = (0 if early_stop else _lib.SA_FLAG_NO_EARLY_STOP) | (_lib.SA_FLAG_BETA0 if beta0 else 0)
        check(self._need("sa_sc_run")(self._sc, int(B), int(T), float(stop_tol), float(freeze_tol), flags))
        self._T_run = int(T)

    def wait(self):
        check(self._need("sa_sc_wait")(self._sc))

    def decide(self, B):
        """Section argmax of the β on the device, (B, L) int32."""
        idx = np.empty((int(B), self.L), dtype=np.int32)
        check(self._need("sa_sc_decide")(self._sc, int(B), idx.ctypes.data_as(self._I32)))
        return idx

    def iters(self, B):
        """Stop index of each codeword of the last run (T when the loop ran out)."""
        it = np.empty(int(B), dtype=np.int32)
        check(self._need("sa_sc_fetch")(self._sc, int(B), None, it.ctypes.data_as(_lib.ct.POINTER(_lib.ct.c_int)), None))
        return it

    def fetch_beta(self, B):
        """The β on the device, (B, L*M)."""
        out = np.empty((int(B), self.L * self.M))
        check(self._need("sa_sc_fetch")(self._sc, int(B), dptr(out), None, None))
        return out

    def fetch_phi(self, B, T):
        """The φ trace of the last run (of T iterations), (B, T, R)."""
        assert int(T) == getattr(self, "_T_run", None), "T must be the last run's"
        phi = np.zeros((int(B), int(T), self.R))
        check(self._need("sa_sc_fetch")(self._sc, int(B), None, None, dptr(phi)))
        return phi

    def llr(self, B, l0, ns, out=None, mode="reference", clip=None):
        """LDPC-bit LLRs of sections [l0, l0+ns) of the β on the device (SparcOperator.llr)."""
        m = llr_mode(mode)
        lgm = int(np.log2(self.M))
        if out is None:
            out = np.empty((B, ns * lgm))
        p, fl = SparcOperator._ptr(out)
        check(self._need("sa_sc_llr")(self._sc, int(B), int(l0), int(ns), p, fl, m,
                                      float("inf") if clip is None else float(clip)))
        return out

    def soft_beta0(self, B, l0, ns, app):
        """β₀ = β with sections [l0, l0+ns) from the LDPC app (SparcOperator.soft_beta0)."""
        if not isinstance(app, int):
            app = as_f64(app)
        p, fl = SparcOperator._ptr(app)
        check(self._need("sa_sc_soft_beta0")(self._sc, int(B), int(l0), int(ns), p, fl))

    def hard_cancel(self, B, l0, ns, app):
        """Hard LDPC decisions of sections [l0, l0+ns) -> (B, ns) indices (SparcOperator.hard_cancel with no dst:
        a coupled design has no shortened operator to cancel into)."""
        if not isinstance(app, int):
            app = as_f64(app)
        p, fl = SparcOperator._ptr(app)
        idx = np.empty((int(B), int(ns)), dtype=np.int32)
        check(self._need("sa_sc_hard_indices")(self._sc, int(B), int(l0), int(ns), p, fl, idx.ctypes.data_as(self._I32)))
        return idx

    def stage_onehot(self, idx):
        """Stage the one-hot β₀ of section indices idx (B, L) for run(..., beta0=True)."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert idx.ndim == 2 and idx.shape[1] == self.L
        check(self._need("sa_sc_stage_onehot")(self._sc, idx.shape[0], idx.ctypes.data_as(self._I32)))


class ScAbOp:
    """``Ab(β)`` -> A β, (n, 1) float64, for the coupled design."""

    def __init__(self, op: CoupledOperator):
        self.op = op

    def __call__(self, b):
        b = np.asarray(b)
        assert b.size == self.op.L * self.op.M
        return self.op.Ab_batch(b.reshape(1, -1)).reshape(-1, 1)


class ScAzOp:
    """``Az(z)`` -> Aᵀ z, (L*M, 1) float64, for the coupled design."""

    def __init__(self, op: CoupledOperator):
        self.op = op

    def __call__(self, z):
        z = np.asarray(z)
        assert z.size == self.op.n
        return self.op.Az_batch(z.reshape(1, -1)).reshape(-1, 1)


def sc_transforms(L, M, n, W, seed=0, *, precision=None, device=None):
    """The coupled design of base matrix W over sparc_transforms(L, M, n, seed)'s
    operator: returns (Ab, Az, ordering), callables like AbOp / AzOp."""
    ordering = make_ordering(L, M, n, seed)
    parent = _cached_operator(L, M, n, ordering, "hadamard", precision, device)
    op = CoupledOperator(parent, W)
    return ScAbOp(op), ScAzOp(op), ordering


def _coupled(Ab) -> CoupledOperator:
    op = getattr(Ab, "op", None)
    if not isinstance(op, CoupledOperator):
        raise TypeError("Ab must come from sc_transforms (a coupled device operator); there is no host fallback")
    return op


def amp_sc_batch(y, Pl, T, Ab, *, early_stop=True, stop_tol=0.0, freeze_tol=0.0, return_live=False, beta0=None):
    """Coupled AMP of B codewords y (B, n): -> (β̂ (B, L*M), iters (B,), φ (B, T, R)),
    with return_live also live (B, T, C) uint8 (CoupledOperator.amp_batch); beta0 (B, L*M): the start."""
    return _coupled(Ab).amp_batch(y, Pl, T, early_stop=early_stop, stop_tol=stop_tol, freeze_tol=freeze_tol,
                                  return_live=return_live, beta0=beta0)


def _start(beta, LM):
    """amp()'s β argument: None or the reference's np.array([None]) sentinel (the zero start), else (L*M,) or (L*M, 1)."""
    if beta is None:
        return None
    b = np.asarray(beta)
    if b.dtype == object and b.size == 1 and b.reshape(-1)[0] is None:
        return None
    b = as_f64(b)
    if b.size != LM or b.ndim > 2 or (b.ndim == 2 and b.shape[1] != 1):
        raise ValueError("beta must be (L*M,) or (L*M, 1)")
    return b.reshape(1, -1)


def amp_sc(y, Pl, L, M, T, Ab, Az, beta=None, *, early_stop=True, stop_tol=0.0, freeze_tol=0.0, return_live=False):
    """Coupled AMP of one codeword, in amp()'s argument order: -> β̂, (L*M, 1);
    with return_live -> (β̂, live (T, C) uint8).  beta: the start β₀ (β = β₀, z = y − A β₀), (L*M,) or (L*M, 1);
    None or np.array([None]) is the zero start."""
    op = _coupled(Ab)
    assert (op.L, op.M) == (int(L), int(M)), "L, M must be the operator's"
    if getattr(Az, "op", None) is not op:
        raise TypeError("Ab and Az must come from one sc_transforms call")
    y = as_f64(y).reshape(1, -1)
    res = op.amp_batch(y, Pl, T, early_stop=early_stop, stop_tol=stop_tol, freeze_tol=freeze_tol, return_live=return_live,
                       beta0=_start(beta, op.L * op.M))
    out = res[0].reshape(-1, 1)
    return (out, res[3][0]) if return_live else out


def mc_decode_sc(Ab, Pl, sigma, T, seeds, batch=256, early_stop=True, stop_tol=0.0, freeze_tol=0.0, return_live=False):
    """Monte-Carlo reps on the coupled design, drawn as harness._draw_reps draws
    them (RandomState(s).randint(0, M, L), then .randn(n) * σ), encoded, decoded
    and decided on the device in batches of `batch`:
    -> (bit errors (R,), stop indices (R,), decisions (R, L)), all int32, and
    with return_live the live trace (R, T, C) uint8 behind them."""
    from .harness import draw_reps
    op = _coupled(Ab)
    seeds = seed_array(seeds)
    nrep = len(seeds)
    errs = np.empty(nrep, dtype=np.int32)
    its = np.empty(nrep, dtype=np.int32)
    dec = np.empty((nrep, op.L), dtype=np.int32)
    live = np.zeros((nrep, int(T), op.C), dtype=np.uint8) if return_live else None
    for i0 in range(0, nrep, int(batch)):
        sl = slice(i0, min(nrep, i0 + int(batch)))
        idx, noise = draw_reps(seeds[sl], op.L, op.M, op.n, float(sigma))
        res = op.mc(idx, noise, Pl, T, early_stop=early_stop, stop_tol=stop_tol, freeze_tol=freeze_tol,
                    return_live=return_live)
        dec[sl], its[sl], errs[sl] = res[0], res[1], res[2]
        if return_live:
            live[sl] = res[4]
    return (errs, its, dec, live) if return_live else (errs, its, dec)
