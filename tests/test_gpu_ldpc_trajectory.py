"""GPU: every belief-propagation kernel instance (DESIGN.md §10's instance
table) against the NumPy oracle at fixed iteration counts: decodes cut at
max_iter = k around the tail hand-offs, with the tail off, at 1, at 3 and at
its default, sized on the host (lb_decode) and on the device (lb_run), on
words that stop before, at and after each hand-off, never converge, belong to
no codeword, carry erased bits of either sign of zero, or are saturated.

Bars: iteration counts exact; minsum app bit-equal (the kernel and the oracle
perform the same IEEE operations in the same order, no transcendental);
sumprod2 / sumprod within the suite's TOL (rtol = atol).  The words' seeds
were chosen from the oracle alone (tests/ldpc_cases.py), and what they must
satisfy is asserted here from the oracle alone."""
import ctypes as ct

import numpy as np
import pytest

import ldpc_cases as lc
from test_gpu_ldpc import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bp():
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible: -m gpu tests need an MI355X"
    return ldpc


class _Worst:
    """Largest deviation from the oracle seen in a test, relative to max(1, |app|) (printed: DESIGN.md §10)."""

    def __init__(self):
        self.dev = 0.0

    def compare(self, algo, app, it, rapp, rit, what):
        assert np.array_equal(it, rit), (what, it, rit)
        if algo == "minsum":
            assert np.array_equal(app, rapp), (what, np.argwhere(app != rapp)[:4])
            return
        with np.errstate(invalid="ignore"):
            d = np.abs(app - rapp) / np.maximum(1.0, np.abs(rapp))
        self.dev = max(self.dev, float(np.max(np.where(app == rapp, 0.0, d))))
        np.testing.assert_allclose(app, rapp, rtol=TOL[algo], atol=TOL[algo], err_msg=str(what))


def _device_sized(bp, c, ch, algo, k):
    B = ch.shape[0]
    c.device_buffers(B)
    lib = bp.load_bp_library()
    assert lib.lb_stage(c._context(), B, np.ascontiguousarray(ch).ctypes.data_as(ct.POINTER(ct.c_double))) == 0
    c.run_buffers(B, algo, max_iter=k)
    return c.fetch_buffers(B)


@pytest.mark.parametrize("algo", lc.ALGOS)
@pytest.mark.parametrize("cell", list(lc.CELLS))
def test_truncated_decodes_against_oracle(bp, cell, algo):
    ref = lc.reference(cell, algo)
    ref.check_preconditions(cell, algo)
    W = len(ref.CH)
    c = lc.make_code(cell)
    info = c.info()
    max_cdeg, max_vdeg, lds, fixed, threads = lc.CELLS[cell][1]
    got = (info["max_cdeg"], info["lds_messages"], info["fixed_dc"], info["threads"])
    assert got == (max_cdeg, lds, fixed, threads)
    assert info["max_vdeg"] == c.vdeg.max() and max_vdeg in (None, info["max_vdeg"])
    assert (info["threads"] < c.Nc) == (cell in ("16_1/2_z96", "16_5/6_z300"))  # the strided check loop
    no_tail = cell == "syn_dv13"
    if no_tail:  # a variable of degree 13: nq == 0, no tail launches
        assert info["tail_at"] == 0
        with pytest.raises(bp.LdpcBpError) as e:
            c.set_tail(3)
        assert e.value.code == -5
        tails = (0, -1)
    else:
        assert info["tail_at"] == 8
        tails = (0, 1, 3, -1)
    worst = _Worst()
    try:
        call = 0
        for tail in tails:
            c.set_tail(tail)
            at = c.info()["tail_at"]
            assert at == (0 if no_tail else 8 if tail < 0 else tail)
            for k in lc.KS:
                # another order and another number of words every call
                idx = np.roll(np.arange(W), call)[:W - call % 3] if W > 2 else np.arange(W)[::1 - 2 * (call % 2)]
                call += 1
                app, it = c.decode_batch(ref.CH[idx], algo, max_iter=k)
                worst.compare(algo, app, it, *ref.at(k, idx), ("host-sized", at, k, idx.tolist()))
            if at == 0:
                continue
            # the tail sized on the device: batches whose share of words entering the tail is small, then
            # all (the estimate left by the call before is too small: the kernels stride), then small
            # again (too large: launches past the last running word return at once)
            hard = np.nonzero(ref.its >= at)[0]  # still running after `at` iterations
            easy = np.nonzero(ref.its < at)[0]
            assert len(hard) and (len(easy) or W == 2)
            if not len(easy):
                easy = hard[:1]
            few = np.concatenate([np.repeat(easy[:1], 36), np.resize(hard, 3), easy[:1]])
            batches = (few, np.resize(hard, 40), np.concatenate([np.resize(easy, 10), hard[:2]]))
            for k in (at + 1, lc.K_TRACE):
                for idx in batches:
                    app, it = _device_sized(bp, c, ref.CH[idx], algo, k)
                    worst.compare(algo, app, it, *ref.at(k, idx), ("device-sized", at, k, len(idx)))
    finally:
        c.set_tail(-1)
    print(f"\ntrajectory {cell} {algo}: its={ref.its.tolist()} worst deviation {worst.dev:.3e}")


@pytest.mark.parametrize("algo", lc.ALGOS)
def test_max_iter_zero_returns_the_channel(bp, algo):
    """max_iter = 0: no iteration runs; app = ch (the variable phase on zero
    messages) and 0 iterations, host- and device-sized, in LDS and in HBM."""
    for cell in ("16_1/2_z24", "16_5/6_z300", "syn_dv13"):
        ref = lc.reference(cell, algo)
        c = lc.make_code(cell)
        # a longer decode first, so that the buffers hold something else
        c.decode_batch(ref.CH, algo, max_iter=2)
        app, it = c.decode_batch(ref.CH, algo, max_iter=0)
        assert np.array_equal(app, ref.CH) and np.array_equal(np.signbit(app), np.signbit(ref.CH))
        assert it.shape == (len(ref.CH),) and not it.any()
        rapp, rit = ref.at(0)
        assert np.array_equal(app, rapp) and np.array_equal(it, rit)
        c.decode_batch(ref.CH, algo, max_iter=2)
        app, it = _device_sized(bp, c, ref.CH, algo, 0)
        assert np.array_equal(app, ref.CH) and not it.any()
        with pytest.raises(AssertionError):
            c.decode_batch(ref.CH, algo, max_iter=-1)


def test_mc_blocks_max_iter_zero_counts_channel_errors(bp):
    """lb_mc_run / lb_mc_run_seeds with max_iter = 0 count the channel's own hard-decision errors."""
    from sparc_ldpc_amd import ldpc_mc
    c = bp.code("802.16", "1/2", 24)
    seeds = np.arange(40, 52)
    sigma = 0.9
    u, w = ldpc_mc._draw_blocks(seeds, c.K, c.N, "awgn")
    x = c.encode_batch(u)
    y = (1 - 2 * x) + sigma * w
    assert np.abs(y).min() > 1e-9  # no decision on the edge
    want = ((y < 0) != x).sum(1)
    assert want.min() > 0
    c.mc_blocks(u, w, sigma, batch=5, max_iter=3)  # leaves decoded apps in the buffers
    for batch in (5, 64):
        errs, it = c.mc_blocks(u, w, sigma, batch=batch, max_iter=0)
        assert np.array_equal(errs, want) and not it.any()
        errs, it = c.mc_blocks_seeds(seeds, sigma, batch=batch, max_iter=0)
        assert np.array_equal(errs, want) and not it.any()
    p = 0.08
    _, wb = ldpc_mc._draw_blocks(seeds, 0, c.N, "bsc")
    errs, it = c.mc_blocks(None, wb, p, channel="bsc", batch=7, max_iter=0)
    assert np.array_equal(errs, (wb < p).sum(1)) and not it.any()
