"""Drop-in for the reference's AWGN sweep ldpc/py/ldpc_awgn.py:60-123: per
code, N_MEASUREMENTS operating points with the SNR-stepping heuristic, every
block encoded, sent, decoded and counted on the GPU (ldpc_mc)."""
from __future__ import annotations

import numpy as np

from . import ldpc as _ldpc
from . import ldpc_mc

__all__ = ["sim", "sim_param"]

_RATES = {"1/2": .5, "2/3": 0.6667, "3/4": 0.75, "5/6": 0.83333}  # ldpc_awgn.py:63-72


def _grid(first_z):
    """The reference's 36 (standard, rate, z, ptype) cases from the protograph
    table: 802.16 at ``first_z`` and at 802.11n's three lifting sizes, every
    rate and type, then 802.11n by z and rate."""
    tab = _ldpc._protographs()
    zs = [int(z) for z in tab["802.11n"]]
    out = [("802.16", rate, z, ptype) for z in [first_z] + zs
           for rate, types in tab["z_free"]["802.16"].items() for ptype in types]
    out += [("802.11n", rate, int(z), "A") for z, rates in tab["802.11n"].items() for rate in rates]
    return out


sim_param = _grid(3)  # ldpc_awgn.py:6-43


def sim(standard, rate, z, ptype='A', N_MEASUREMENTS=24, C_AWGN_OFFSET=1.0, P_STEP=100.0,
        MIN_ERRORS=100, MAX_BLOCKS=400000, *, seed0=0, batch=1024, results_file=None, draws="host",
        dectype="sumprod2", stream=False, quant=None):
    """ldpc_awgn.py:60-123.  Starts C_AWGN_OFFSET dB above the SNR of the AWGN
    rate, and per point: sigma2 = 1 / 10**(SNR/10), blocks until MIN_ERRORS
    block errors or MAX_BLOCKS, then SNR += sqrt(P_STEP / nblocks).  Point d
    decodes the blocks seed0 + d * 10_000_000, ... (ldpc_mc's seed contract with
    sigma = sqrt(sigma2)).  Returns the reference's tuples (standard, rate, z,
    SNR, nblocks, nblockerrors, nblocks*K, nbiterrors, nit_total) and appends
    them to ``results_file`` in its line format when given.  draws="device":
    the blocks are drawn on the GPU from their seeds (ldpc_mc).  dectype: the
    decoder (code.decode_batch's names, the layered ones and their binary32
    "_f32" forms included; nit_total then counts sweeps).  stream=True
    (draws="device", a layered dectype): every point as one stream of refilled
    decoder slots (ldpc_mc._mc_point); the same tuples.  quant (None, True or
    (frac_bits, msg_bits, app_bits), with dectype "layered_minsum"): the
    fixed-point decoder (ldpc.code)."""
    ldpc_mc._check_request(draws, stream, dectype, quant)
    if rate not in _RATES:
        raise NameError("Rate unsupported")
    R = _RATES[rate]
    SNR = 10.0 * np.log10(np.power(2, R) - 1.0) + C_AWGN_OFFSET
    code = _ldpc.code(standard, rate, z, ptype)
    K = code.K
    res = []
    for datapoint in range(N_MEASUREMENTS):
        sigma2 = 1 / np.power(10, SNR / 10.0)
        r = ldpc_mc._mc_point(code, float(np.sqrt(sigma2)), "awgn", MIN_ERRORS, MAX_BLOCKS,
                              seed0 + datapoint * 10_000_000, batch, dectype=dectype, draws=draws, stream=stream,
                              quant=quant)
        nblocks = r["blocks"]
        output = (standard, rate, z, SNR, nblocks, r["block_errors"], nblocks * K, r["bit_errors"], r["iters_total"])
        res.append(output)
        if results_file:
            with open(results_file, 'a') as f:
                f.write(str(output))
                f.write("\n")
        SNR += np.sqrt(P_STEP / nblocks)  # heuristic SNR stepping method (:116)
    return res
