"""State evolution (SE) of the AMP decoder on the device (sa_se, csrc/sa_se.hip).

SE is the scalar recursion that predicts a decode without running a codeword:
for an allocation ``Pl`` (``P = Pl.sum()``), section size M, code length n and
noise sigma,

    tau_0^2 = sigma^2 + P,   c_l = sqrt(n Pl_l),   a = c_l / tau_t,
    E_l = E[ e^(a^2 + a U_1) / (e^(a^2 + a U_1) + sum_{j>=2} e^(a U_j)) ],   U_j i.i.d. N(0, 1),
    x_{t+1} = sum_l (Pl_l / P) E_l,   tau_{t+1}^2 = sigma^2 + P (1 - x_{t+1}),

and the predicted section error rate at t is the probability that
``a^2 + a U_1 < max_{j>=2} a U_j``, averaged over the sections.  It is the
decoder's own section softmax (``amp``) applied to ``s = c e_true + tau U``.

The expectation is a mean over ``samples`` rows of M Gaussians.  The same rows
serve every section, every iteration and every allocation of a call (common
random numbers): a call is deterministic, and two allocations are compared on
the same noise, so their difference has far less variance than either value.
Fresh draws per iteration are not offered.  With ``draws="device"`` row s is
``RandomState(seed + s).randn(M)``, drawn on the device.

Spatially coupled SPARCs (``sc.py``) have the same
recursion with one effective-noise level per row block (phi_r) and per column
block (tau_c^2) of the base matrix W: ``sc_state_evolution`` (sa_sc_se), on the
same rows, and ``sc_search`` over (omega, Lambda) as ``pa_search`` is over (a, f).
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass

import numpy as np

from . import _lib

__all__ = ["SEResult", "state_evolution", "se_draws", "PASearch", "pa_search",
           "SCSEResult", "sc_state_evolution", "SCSearch", "sc_search"]


@dataclass
class SEResult:
    """tau2 (B, T+1), x (B, T), ser (B, T) = missed (section, sample) pairs / (L S),
    sections (B, L) = E_l of the last iteration, miss (B, T) the raw counts, ms the
    device time of the draw and the iterations; 1-D when Pl was 1-D."""
    tau2: np.ndarray
    x: np.ndarray
    ser: np.ndarray
    sections: np.ndarray
    miss: np.ndarray
    ms: float


def _device(device):
    if device is not None:
        return int(device)
    from .operators import default_device
    return default_device()


def _seeds(seeds) -> np.ndarray:
    from .operators import seed_array
    return seed_array(list(np.asarray(seeds).reshape(-1)))


def se_draws(seeds, M, device=None) -> np.ndarray:
    """The rows the seeded path of state_evolution uses: row i is
    ``RandomState(seeds[i]).randn(M)`` drawn on the device (NumPy's up to the
    device library's log: about one value in a hundred differs, by under
    2**-49 relative)."""
    lib = _lib.load()
    seeds = _seeds(seeds)
    out = np.empty((len(seeds), int(M)))
    _lib.check(lib.sa_se_draws(_device(device), len(seeds), int(M), seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)),
                               _lib.dptr(out)))
    return out


def state_evolution(Pl, M, n, sigma, T, samples=1024, seed=0, draws="device", device=None) -> SEResult:
    """SE of one allocation (Pl 1-D) or a batch (Pl (B, L); sigma a scalar or (B,)).

    draws: "device" (rows seeded ``seed + arange(samples)``) or an (S, M) array
    of standard Gaussians of the caller's (``samples`` and ``seed`` are then
    unused)."""
    lib = _lib.load()
    Pl = _lib.as_f64(Pl)
    one = Pl.ndim == 1
    if Pl.ndim not in (1, 2):
        raise ValueError("Pl must be 1-D or (B, L)")
    Pl2 = np.ascontiguousarray(Pl.reshape(1, -1) if one else Pl)
    B, L = Pl2.shape
    sig = np.asarray(sigma, dtype=np.float64)
    if sig.ndim == 0:
        sig = np.full(B, float(sig))
    if sig.shape != (B,):
        raise ValueError("sigma must be a scalar or one value per allocation")
    sig = np.ascontiguousarray(sig)
    if isinstance(draws, str):
        if draws != "device":
            raise ValueError('draws must be "device" or an (S, M) array')
        S = int(samples)
        seeds = _seeds(int(seed) + np.arange(max(S, 0), dtype=np.int64))
        p_seeds, p_U = seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), None
    else:
        U = _lib.as_f64(draws)
        if U.ndim != 2 or U.shape[1] != int(M):
            raise ValueError("draws must be an (S, M) array")
        S = U.shape[0]
        p_seeds, p_U = None, _lib.dptr(U)
    T = int(T)
    tau2 = np.zeros((B, max(T, 0) + 1))
    x = np.zeros((B, max(T, 0)))
    miss = np.zeros((B, max(T, 0)), dtype=np.int64)
    sec = np.zeros((B, L))
    ms = ct.c_double(0.0)
    _lib.check(lib.sa_se(_device(device), B, L, int(M), int(n), _lib.dptr(Pl2), _lib.dptr(sig), T, S, p_seeds, p_U,
                         _lib.dptr(tau2), _lib.dptr(x), miss.ctypes.data_as(ct.POINTER(ct.c_int64)), _lib.dptr(sec),
                         ct.cast(ct.pointer(ms), ct.POINTER(ct.c_double))))
    ser = miss / float(L * S)
    if one:
        tau2, x, ser, sec, miss = tau2[0], x[0], ser[0], sec[0], miss[0]
    return SEResult(tau2=tau2, x=x, ser=ser, sections=sec, miss=miss, ms=float(ms.value))


@dataclass
class PASearch:
    """pa_search's grids over (a_values, f_values): the final x, the final ser,
    ``iters`` = the number of iterations after which ser first had its final
    value, and ``best`` = the (a, f) of the largest final x (the first in
    row-major order on ties); ``result`` is the batch's SEResult, allocation
    i * len(f_values) + j for (a_values[i], f_values[j])."""
    a_values: np.ndarray
    f_values: np.ndarray
    x: np.ndarray
    ser: np.ndarray
    iters: np.ndarray
    best: tuple
    result: SEResult


def pa_search(L, M, n, P, sigma, a_values, f_values, T, C=None, **kw) -> PASearch:
    """SE of every ``pa_parameterised(L, C, P, a, f)`` on the grid, as one
    batch on the same Gaussian rows.  C defaults to the capacity
    0.5 log2(1 + P / sigma^2); kw goes to state_evolution (samples, seed,
    draws, device)."""
    from .harness import pa_parameterised
    a_values = np.atleast_1d(np.asarray(a_values, dtype=np.float64))
    f_values = np.atleast_1d(np.asarray(f_values, dtype=np.float64))
    if C is None:
        C = 0.5 * np.log2(1.0 + P / float(sigma) ** 2)
    Pl = np.array([pa_parameterised(L, C, P, a, f) for a in a_values for f in f_values])
    r = state_evolution(Pl, M, n, sigma, T, **kw)
    shape = (len(a_values), len(f_values))
    xf = r.x[:, -1].reshape(shape)
    sf = r.ser[:, -1].reshape(shape)
    iters = ((r.ser == r.ser[:, -1:]).argmax(axis=1) + 1).reshape(shape)
    i, j = np.unravel_index(int(np.argmax(xf)), shape)
    return PASearch(a_values=a_values, f_values=f_values, x=xf, ser=sf, iters=iters,
                    best=(float(a_values[i]), float(f_values[j])), result=r)


@dataclass
class SCSEResult:
    """Coupled SE of one configuration: phi (T+1, R), tau2 (T, C), x (T, C), ser
    (T, C) = the missed (section, sample) pairs of column block c / ((L / C) S),
    ser_all (T,) = all missed pairs / (L S), miss (T, C) the raw counts, stop the
    predicted stop index (the first t >= 1 at which every phi_r^t has the bits of
    phi_r^{t-1}, the decoder's stopping rule; T: none), sections (L,) = E_l of
    the last iteration, ms the device time of the draw and the iterations.

    Of a batch: phi, tau2, x, ser and miss are lists of B such arrays, each of
    its configuration's own R and C (nothing padded); ser_all (B, T), stop (B,),
    sections (B, L); ``config(b)`` is configuration b's own SCSEResult."""
    phi: object
    tau2: object
    x: object
    ser: object
    ser_all: np.ndarray
    miss: object
    stop: object
    sections: np.ndarray
    ms: float

    def config(self, b) -> "SCSEResult":
        if not isinstance(self.phi, list):
            raise ValueError("not a batch")
        return SCSEResult(phi=self.phi[b], tau2=self.tau2[b], x=self.x[b], ser=self.ser[b], ser_all=self.ser_all[b],
                          miss=self.miss[b], stop=int(self.stop[b]), sections=self.sections[b], ms=self.ms)


def _per_config(v, B, what, dtype):
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        a = np.full(B, a[()], dtype=dtype)
    if a.shape != (B,):
        raise ValueError(f"{what} must be a scalar or one value per configuration")
    return np.ascontiguousarray(a)


def sc_state_evolution(Pl, M, n, W, sigma, T, samples=1024, seed=0, draws="device", device=None, skip=True) -> SCSEResult:
    """Coupled SE of one configuration (Pl 1-D, W an R x C base matrix) or of a
    batch (Pl (B, L); W a list of B base matrices, or one for all; n and sigma
    scalars or one value per configuration), all on the same Gaussian rows.

    draws as in state_evolution.  skip=False recomputes the column blocks whose
    tau_c^2 did not change from one iteration to the next (the same bits)."""
    lib = _lib.load()
    if not hasattr(lib, "sa_sc_se"):
        raise _lib.SparcAmpError(_lib.SA_ERR_UNSUPPORTED, "this build of the library has no sa_sc_se")
    Pl = _lib.as_f64(Pl)
    one = Pl.ndim == 1
    if Pl.ndim not in (1, 2):
        raise ValueError("Pl must be 1-D or (B, L)")
    Pl2 = np.ascontiguousarray(Pl.reshape(1, -1) if one else Pl)
    B, L = Pl2.shape
    if isinstance(W, np.ndarray) and W.ndim == 2 or one:
        Ws = [_lib.as_f64(W)] * B
    else:
        Ws = [_lib.as_f64(w) for w in W]
    if len(Ws) != B or any(w.ndim != 2 or w.size == 0 for w in Ws):
        raise ValueError("W must be a 2-d base matrix (R x C), or one per configuration")
    ns = _per_config(n, B, "n", np.int32)
    sig = _per_config(sigma, B, "sigma", np.float64)
    Rs = np.array([w.shape[0] for w in Ws], dtype=np.int32)
    Cs = np.array([w.shape[1] for w in Ws], dtype=np.int32)
    Wcat = np.ascontiguousarray(np.concatenate([w.reshape(-1) for w in Ws]))
    if isinstance(draws, str):
        if draws != "device":
            raise ValueError('draws must be "device" or an (S, M) array')
        S = int(samples)
        seeds = _seeds(int(seed) + np.arange(max(S, 0), dtype=np.int64))
        p_seeds, p_U = seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), None
    else:
        U = _lib.as_f64(draws)
        if U.ndim != 2 or U.shape[1] != int(M):
            raise ValueError("draws must be an (S, M) array")
        S = U.shape[0]
        p_seeds, p_U = None, _lib.dptr(U)
    T = int(T)
    Tn = max(T, 0)
    Rmax, Cmax = int(Rs.max()), int(Cs.max())
    phi = np.zeros((B, Tn + 1, Rmax))
    tau2 = np.zeros((B, Tn, Cmax))
    x = np.zeros((B, Tn, Cmax))
    miss = np.zeros((B, Tn, Cmax), dtype=np.int64)
    stop = np.zeros(B, dtype=np.int32)
    sec = np.zeros((B, L))
    ms = ct.c_double(0.0)
    ip = ct.POINTER(ct.c_int)
    _lib.check(lib.sa_sc_se(_device(device), B, L, int(M), ns.ctypes.data_as(ip), Rs.ctypes.data_as(ip),
                            Cs.ctypes.data_as(ip), _lib.dptr(Wcat), _lib.dptr(Pl2), _lib.dptr(sig), T, S, p_seeds, p_U,
                            Rmax, Cmax, 0 if skip else _lib.SA_SCSE_NO_SKIP, _lib.dptr(phi), _lib.dptr(tau2), _lib.dptr(x),
                            miss.ctypes.data_as(ct.POINTER(ct.c_int64)), stop.ctypes.data_as(ip), _lib.dptr(sec),
                            ct.cast(ct.pointer(ms), ct.POINTER(ct.c_double))))
    phis = [phi[b, :, :Rs[b]].copy() for b in range(B)]
    tau2s = [tau2[b, :, :Cs[b]].copy() for b in range(B)]
    xs = [x[b, :, :Cs[b]].copy() for b in range(B)]
    misses = [miss[b, :, :Cs[b]].copy() for b in range(B)]
    sers = [misses[b] / float((L // Cs[b]) * S) for b in range(B)]
    ser_all = miss.sum(axis=2) / float(L * S)
    r = SCSEResult(phi=phis, tau2=tau2s, x=xs, ser=sers, ser_all=ser_all, miss=misses, stop=stop.astype(np.int64),
                   sections=sec, ms=float(ms.value))
    return r.config(0) if one else r


@dataclass
class SCSearch:
    """sc_search's grids over (omega_values, Lambda_values): ``n`` the code
    length each pair ran at, ``rate`` = L log2(M) / n, the final ``ser`` (all
    sections), the predicted ``stop`` index, ``iters`` = the number of
    iterations after which ser first had its final value, and ``best`` = the
    (omega, Lambda) of the lowest final ser, then the smallest stop index, then
    the first in row-major order; ``result`` is the batch's SCSEResult,
    configuration i * len(Lambda_values) + j for (omega_values[i], Lambda_values[j])."""
    omega_values: np.ndarray
    Lambda_values: np.ndarray
    n: np.ndarray
    rate: np.ndarray
    ser: np.ndarray
    stop: np.ndarray
    iters: np.ndarray
    best: tuple
    result: SCSEResult


def sc_search(L, M, n, P, sigma, omega_values, Lambda_values, T, **kw) -> SCSearch:
    """Coupled SE of every ``base_matrix(omega, Lambda)`` on the grid with the
    flat allocation P / L, as one batch on the same Gaussian rows.  A pair runs
    at the code length R ceil(n / R), R = Lambda + omega - 1: the smallest
    multiple of R not below n, so that no pair runs above the asked rate.  A
    pair whose Lambda does not divide L or whose R is above SA_SC_MAX_BLOCKS
    raises ValueError.  kw goes to sc_state_evolution (samples, seed, draws,
    device, skip)."""
    from .sc import base_matrix
    omega_values = np.atleast_1d(np.asarray(omega_values, dtype=np.int64))
    Lambda_values = np.atleast_1d(np.asarray(Lambda_values, dtype=np.int64))
    L, n = int(L), int(n)
    Ws, ns = [], []
    for om in omega_values:
        for lam in Lambda_values:
            om, lam = int(om), int(lam)
            if om < 1 or lam < 1:
                raise ValueError(f"(omega, Lambda) = ({om}, {lam}): both must be at least 1")
            R = lam + om - 1
            if L % lam != 0:
                raise ValueError(f"(omega, Lambda) = ({om}, {lam}): Lambda does not divide L = {L}")
            if R > _lib.SA_SC_MAX_BLOCKS:
                raise ValueError(f"(omega, Lambda) = ({om}, {lam}): R = {R} row blocks, above SA_SC_MAX_BLOCKS = "
                                 f"{_lib.SA_SC_MAX_BLOCKS}")
            Ws.append(base_matrix(om, lam))
            ns.append(R * -(-n // R))
    Pl = np.full((len(Ws), L), float(P) / L)
    r = sc_state_evolution(Pl, M, ns, Ws, sigma, T, **kw)
    shape = (len(omega_values), len(Lambda_values))
    sf = r.ser_all[:, -1].reshape(shape)
    stop = np.asarray(r.stop).reshape(shape)
    iters = ((r.ser_all == r.ser_all[:, -1:]).argmax(axis=1) + 1).reshape(shape)
    order = sorted(range(len(Ws)), key=lambda q: (sf.reshape(-1)[q], stop.reshape(-1)[q], q))
    i, j = np.unravel_index(order[0], shape)
    n_grid = np.array(ns, dtype=np.int64).reshape(shape)
    return SCSearch(omega_values=omega_values, Lambda_values=Lambda_values, n=n_grid,
                    rate=L * np.log2(M) / n_grid, ser=sf, stop=stop, iters=iters,
                    best=(int(omega_values[i]), int(Lambda_values[j])), result=r)
