"""Drop-in for the reference's BSC sweep ldpc/ldpc_bsc.py:63-113: the all-zero
word through a binary symmetric channel at ten crossover probabilities,
``repeats`` blocks each, decoded and counted on the GPU (ldpc_mc)."""
from __future__ import annotations

import numpy as np

from . import ldpc as _ldpc
from . import ldpc_mc
from .ldpc_awgn import _grid

__all__ = ["sim", "sim_param"]

# the crossover probability whose capacity equals the rate (ldpc_bsc.py:67-78)
_P0 = {"1/2": 0.11, "2/3": 0.06, "5/6": 0.02459, "3/4": 0.0415}

sim_param = _grid(100)  # ldpc_bsc.py:6-43


def sim(standard, rate, z, ptype='A', *, repeats=100, seed0=0, draws="host", dectype="sumprod2", stream=False,
        quant=None):
    """ldpc_bsc.py:63-113: (res, parray) with parray = linspace(p0, 0.001, 10)
    and res[i] the mean bit error rate of ``repeats`` blocks at parray[i].
    Point i decodes the blocks seed0 + i * 10_000_000, ... (ldpc_mc's BSC
    contract: random_sample(N) < p flips the bit).  draws="device": the
    uniform values are drawn on the GPU from the seeds (the same values).
    dectype: the decoder (code.decode_batch's names, the layered ones and their
    binary32 "_f32" forms included).  stream=True (draws="device", a layered
    dectype): the blocks through refilled decoder slots (ldpc_mc.mc_ldpc); the
    same results.  quant (None, True or (frac_bits, msg_bits, app_bits), with
    dectype "layered_minsum"): the fixed-point decoder (ldpc.code)."""
    ldpc_mc._check_request(draws, stream, dectype, quant)
    if rate not in _P0:
        raise NameError("Rate unsupported")
    p = _P0[rate]
    code = _ldpc.code(standard, rate, z, ptype)
    N = code.N
    res = []
    parray = np.linspace(p, 0.001, 10)
    for i, q in enumerate(parray):
        base = seed0 + i * 10_000_000
        be, _ = ldpc_mc.mc_ldpc(code, float(q), range(base, base + repeats), channel="bsc", dectype=dectype, draws=draws,
                                stream=stream, quant=quant)
        errors = [int(b) / N for b in be]
        res.append(np.sum(errors) / repeats)
    return res, parray
