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
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass

import numpy as np

from . import _lib

__all__ = ["SEResult", "state_evolution", "se_draws", "PASearch", "pa_search"]


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
