"""LDPC-only Monte-Carlo on the device: the reference's ``sim_ldpc``
(ldpc/sparc_ldpc.py:1064-1124) and the loops of ldpc/py/ldpc_awgn.py:60-123 and
ldpc/ldpc_bsc.py:63-113 with the encoder, the channel, belief propagation and
the error count on the GPU (csrc/ldpc_mc.hip); two ints per block come back.

A block is its seed ``s`` in [0, 2**32).  With ``rs = np.random.RandomState(s)``:

* AWGN, standard code (802.11n / 802.16): ``u = rs.randint(0, 2, K)``, then
  ``w = rs.randn(N)``; ``x = encode(u)``;
  ``ch = (2.0 / sigma**2) * ((1.0 - 2.0*x) + sigma*w)`` in that operation order.
* AWGN, any other standard: ``x = 0`` and ``w = rs.randn(N)`` only (the
  reference's all-zero branch, sparc_ldpc.py:1098-1102).
* BSC, crossover ``p``: ``x = 0``, ``y = rs.random_sample(N) < p``,
  ``ch = -log((1-p)/p)`` where y is set and ``+log((1-p)/p)`` elsewhere
  (ldpc_bsc.py:52-56).
* Per block: ``bit_errors = sum((app < 0) != x)`` over all N bits, and the
  decoder's iteration count.

``_draw_blocks`` is that definition in NumPy; ``draw_blocks`` is its native
twin on the host cores (lb_draw_blocks), bit for bit.  Results do not depend
on the batch size, the rank count or the order the blocks are decoded in.

``draws="device"`` (mc_ldpc and everything above it) draws the blocks on the
GPU from their seeds instead (lb_mc_run_seeds: only the seeds go up);
``draw_blocks_device`` returns those blocks.  The bits and the BSC's uniform
values are the host's bit for bit; the AWGN noise is the host's up to the
device library's ``log`` (a few values in a thousand differ, by under 2**-49
relative), so an AWGN block's result may differ from its host-drawn one.

``stream=True`` (with ``draws="device"``, a layered ``dectype`` and one rank)
runs an operating point as one stream (code.mc_stream_seeds,
lb_mc_stream_seeds): chunks of blocks on two lanes, each chunk decoded and
counted by one persistent kernel whose workgroups take the blocks by ticket,
so a block that does not converge holds one CU and not a batch.  The stopping
rule runs on the device and the host; per block and per point the results are
the batch path's.
"""
from __future__ import annotations

import ctypes as ct
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import ldpc as _ldpc
from .harness import LDPCParams, ber_point, consume_in_seed_order, draw_threads
from .operators import seed_array as _seed_array  # uint32 seeds; ValueError outside [0, 2**32), no masking

__all__ = ["draw_blocks", "draw_blocks_device", "mc_ldpc", "sim_ldpc_mc", "info_bits"]

_STANDARD = ("802.11n", "802.16")  # the codes the reference encodes (sparc_ldpc.py:1098)
_RATES = {"1/2": .5, "2/3": 0.6667, "3/4": 0.75, "5/6": 0.83333, "0.45": 0.45}  # sparc_ldpc.py:1075-1086


def _check_request(draws, stream, dectype, quant, world=1) -> bool:
    """What every entry here checks of its keywords before any library call:
    draws; stream=True (the blocks through refilled decoder slots,
    code.mc_stream_seeds) goes with device draws, a layered decoder and one
    rank; the decoder's name; quant (ldpc._quant_widths).  Returns ``stream``."""
    if draws not in ("host", "device"):
        raise ValueError('draws must be "host" or "device"')
    if stream:
        if draws != "device":
            raise ValueError('stream=True needs draws="device"')
        if not str(dectype).startswith("layered_"):
            raise ValueError("stream=True needs a layered dectype")
        if world != 1:
            raise ValueError("stream=True runs on one rank (world == 1)")
    if dectype not in _ldpc._ALGOS:
        raise NameError("Decoder type unknonwn")
    _ldpc._quant_widths(quant, dectype)
    return bool(stream)


def info_bits(code, channel="awgn") -> int:
    """K of the blocks drawn for ``code``: its information length where the
    reference encodes (AWGN, 802.11n / 802.16), 0 for the all-zero word."""
    return code.K if channel == "awgn" and code.standard in _STANDARD else 0


def _draw_arrays(seeds, K, N, channel):
    """What the three draw functions start from: the channel checked, the seeds
    as uint32, and u (B, K) uint8 (None when K == 0) and w (B, N) float64 to fill."""
    if channel not in _ldpc._CHANNELS:
        raise ValueError(f"channel must be one of {sorted(_ldpc._CHANNELS)}")
    seeds = _seed_array(seeds)
    K, N = int(K), int(N)
    return seeds, K, N, (np.empty((len(seeds), K), dtype=np.uint8) if K else None), np.empty((len(seeds), N))


def _draw_blocks(seeds, K, N, channel="awgn"):
    """The seed contract in NumPy: (u (B, K) uint8 or None when K == 0,
    w (B, N) float64) — randint(0, 2, K) then randn(N) ("awgn") or
    random_sample(N) ("bsc") of RandomState(s) per block."""
    seeds, K, N, u, w = _draw_arrays(seeds, K, N, channel)
    for i, s in enumerate(seeds):
        rs = np.random.RandomState(int(s))
        if K:
            u[i] = rs.randint(0, 2, K)
        w[i] = rs.randn(N) if channel == "awgn" else rs.random_sample(N)
    return u, w


def draw_blocks(seeds, K, N, channel="awgn", threads=None):
    """_draw_blocks, bit for bit, by libldpc_bp's native restatement of NumPy's
    legacy generator over at most draw_threads() host threads
    (lb_draw_blocks).  Needs no device; releases the GIL."""
    seeds, K, N, u, w = _draw_arrays(seeds, K, N, channel)
    lib = _ldpc.load_bp_library()
    _ldpc._check(lib.lb_draw_blocks(seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), len(seeds), K, N,
                                    _ldpc._CHANNELS[channel], None if u is None else u.ctypes.data_as(_ldpc._U8),
                                    w.ctypes.data_as(_ldpc._D), draw_threads() if threads is None else int(threads)))
    return u, w


def draw_blocks_device(code, seeds, channel="awgn"):
    """The blocks mc_ldpc(draws="device") decodes: _draw_blocks' (u, w) for
    ``code`` (K = info_bits, N = code.N) drawn on the GPU from their seeds
    (lb_draw_blocks_device) and copied back."""
    seeds, K, N, u, w = _draw_arrays(seeds, info_bits(code, channel), code.N, channel)
    lib = _ldpc.load_bp_library()
    _ldpc._check(lib.lb_draw_blocks_device(code._context(), seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)), len(seeds),
                                           K, N, _ldpc._CHANNELS[channel],
                                           None if u is None else u.ctypes.data_as(_ldpc._U8),
                                           w.ctypes.data_as(_ldpc._D)))
    return u, w


def mc_ldpc(code, a, seeds, channel="awgn", batch=1024, dectype="sumprod2", drawn=None, draws="host", stream=False,
            quant=None):
    """Blocks ``seeds`` of ``code`` at sigma (AWGN) or p (BSC) ``a``: per-block
    int64 (bit_errors, iters) in seed order.  ``drawn``: the blocks' (u, w)
    when the caller has drawn them already (draw_blocks).  draws="device":
    the blocks are drawn on the GPU from their seeds (code.mc_blocks_seeds).
    stream=True (device draws, a layered dectype): the same results through
    code.mc_stream_seeds, ``batch`` being its chunk.  quant (with dectype
    "layered_minsum"): the fixed-point decoder, see ldpc.code."""
    _check_request(draws, stream, dectype, quant)
    seeds = list(seeds)
    if draws == "device":
        if drawn is not None:
            raise ValueError('drawn blocks go with draws="host"')
        seeds = _seed_array(seeds)
    if not len(seeds):
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    if stream:
        return code.mc_stream_seeds(seeds, a, channel, batch, dectype, quant=quant)[:2]
    if draws == "device":
        return code.mc_blocks_seeds(seeds, a, channel, batch, dectype, quant=quant)
    u, w = draw_blocks(seeds, info_bits(code, channel), code.N, channel) if drawn is None else drawn
    return code.mc_blocks(u, w, a, channel, batch, dectype, quant=quant)


def _mc_point(code, a, channel, min_errors, max_blocks, seed_base, batch, dectype="sumprod2", rank=0, world=1,
              allreduce=None, timings=None, draws="host", stream=False, quant=None):
    """One operating point by the reference's stopping rule (harness.ber_point)
    over the blocks seed_base, seed_base + 1, ...: round r + 1 is drawn in a
    worker thread while round r decodes.  ``timings`` (a dict) receives the
    seconds spent drawing and the device milliseconds of the decodes.
    draws="device": every round is drawn on the GPU in front of its decode,
    and no worker thread is started.
    stream=True (device draws, a layered dectype, world == 1): one call of
    code.mc_stream_seeds over seed_base + arange(max_blocks) with the rule on
    the device (``batch`` is its chunk), and the result from its first blocks
    by the same sequential arithmetic (harness.consume_in_seed_order): the
    same dict as stream=False.  ``timings["stream"]`` receives the call's
    info (used, decoded, slots, chunks).  quant: as mc_ldpc."""
    if _check_request(draws, stream, dectype, quant, world):
        nblk = max(1, int(max_blocks))
        be, it, info = code.mc_stream_seeds(int(seed_base) + np.arange(nblk, dtype=np.int64), a, channel, batch,
                                            dectype, min_errors=int(min_errors), quant=quant)
        if timings is not None:
            timings["draw_s"] = timings.get("draw_s", 0.0)  # (inside device_ms)
            timings["device_ms"] = timings.get("device_ms", 0.0) + code.mc_event_ms()
            timings["stream"] = info
        return consume_in_seed_order(be, it, code.N, min_errors, max_blocks)
    from .dist import shard_seeds
    if draws == "device":
        ms = [0.0]

        def decode_seeds(seeds):
            out = mc_ldpc(code, a, seeds, channel, batch, dectype, draws="device", quant=quant)
            ms[0] += code.mc_event_ms()
            return out

        res = ber_point(decode_seeds, code.N, min_errors, max_blocks, batch, rank, world, allreduce,
                        seed_base=seed_base)
        if timings is not None:
            timings["draw_s"] = timings.get("draw_s", 0.0)  # (inside device_ms)
            timings["device_ms"] = timings.get("device_ms", 0.0) + ms[0]
        return res
    K, N = info_bits(code, channel), code.N
    max_rounds = -(-int(max_blocks) // (batch * world))
    pending = {}
    state = dict(rnd=0, draw_s=0.0, device_ms=0.0)

    def draw(seeds):
        t0 = time.perf_counter()
        out = draw_blocks(seeds, K, N, channel)
        state["draw_s"] += time.perf_counter() - t0
        return out

    with ThreadPoolExecutor(max_workers=1) as pool:
        def decode_round(seeds):
            r = state["rnd"]
            state["rnd"] = r + 1
            fut = pending.pop(r, None)
            drawn = fut.result() if fut is not None else draw(seeds)
            if r + 1 < max_rounds:
                pending[r + 1] = pool.submit(draw, shard_seeds(seed_base, r + 1, batch, rank, world))
            out = mc_ldpc(code, a, seeds, channel, batch, dectype, drawn=drawn, quant=quant)
            if timings is not None:
                state["device_ms"] += code.mc_event_ms()
            return out

        res = ber_point(decode_round, N, min_errors, max_blocks, batch, rank, world, allreduce, seed_base=seed_base)
    if timings is not None:
        timings["draw_s"] = timings.get("draw_s", 0.0) + state["draw_s"]
        timings["device_ms"] = timings.get("device_ms", 0.0) + state["device_ms"]
    return res


def sim_ldpc_mc(ldpcparams: LDPCParams, sigma, MIN_ERRORS=100, MAX_BLOCKS=400000, seed0=0, batch=1024, rank=0,
                world=1, allreduce=None, timings=None, draws="host", dectype="sumprod2", stream=False, quant=None):
    """sim_ldpc (sparc_ldpc.py:1064-1124) over the blocks seed0, seed0 + 1, ...
    with everything but the draws on the device: blocks until MIN_ERRORS block
    errors or MAX_BLOCKS blocks, consumed in seed order whatever ``batch`` and
    ``world``.  Returns dict(ber, blocks, block_errors, bit_errors, nit_total)
    with ber = bit_errors / (blocks * N) from the integer counts (:1119).
    draws="device": the draws on the device too (only the seeds go up).
    dectype: the decoder (code.decode_batch's names; with a layered one
    nit_total counts sweeps; "layered_sumprod2_f32" / "layered_minsum_f32"
    decode on binary32 messages).
    stream=True (draws="device", a layered dectype, world == 1): the point as
    one stream of refilled decoder slots (_mc_point); the same dict.
    quant (None, True or (frac_bits, msg_bits, app_bits), with dectype
    "layered_minsum"): the fixed-point decoder (ldpc.code)."""
    _check_request(draws, stream, dectype, quant, world)
    if ldpcparams.r_ldpc not in _RATES:
        raise NameError("Rate unsupported")
    code = _ldpc.code(ldpcparams.standard, ldpcparams.r_ldpc, ldpcparams.z, ldpcparams.ptype)
    r = _mc_point(code, float(sigma), "awgn", MIN_ERRORS, MAX_BLOCKS, seed0, batch, dectype, rank, world,
                  allreduce, timings, draws, stream, quant)
    return dict(ber=r["bit_errors"] / (r["blocks"] * code.N), blocks=r["blocks"], block_errors=r["block_errors"],
                bit_errors=r["bit_errors"], nit_total=r["iters_total"])
