"""GPU: LDPC blocks drawn on the device from their seeds
(lb_draw_blocks_device / lb_mc_run_seeds, csrc/legacy_mt_dev.h) against NumPy
(ldpc_mc._draw_blocks), and the device pipeline on such draws against the same
pipeline on the same arrays sent up from the host.

The bits and the BSC's uniform values have no log in them: exact.  The AWGN
noise is held to 2**-49 relative, the bar derived in test_gpu_mc_draws.py
(here without the product with sigma)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 2.0 ** -49
SEEDS = [0, 1, 2 ** 31, 2 ** 32 - 1] + list(range(1000, 1007))  # 11 blocks
MC_SEEDS = list(range(100, 137))  # 37 blocks: batch 16 gives two full batches and a partial one

# (standard, rate, z): K = 324 of N = 648 (the trials straddle the 624-word
# blocks), K = 160 of N = 192 (aligned), and a code the reference does not
# encode (K = 0: no randint, the noise starts at word 0)
CODES = [("802.11n", "1/2", 27), ("802.16", "5/6", 8), ("2_7_12_good", "1/2", 16)]
# sigma at which some of MC_SEEDS' blocks fail and some do not
SIGMA = {("802.11n", "1/2", 27): 0.85, ("802.16", "5/6", 8): 0.56}

_codes, _dev = {}, {}


def _code(std, rate, z):
    from sparc_ldpc_amd import ldpc
    if (std, rate, z) not in _codes:
        _codes[(std, rate, z)] = ldpc.code(std, rate, z)
    return _codes[(std, rate, z)]


def _device_blocks(key, seeds, channel):
    """draw_blocks_device of a case, drawn once"""
    from sparc_ldpc_amd import ldpc_mc
    k = (key, tuple(seeds), channel)
    if k not in _dev:
        _dev[k] = ldpc_mc.draw_blocks_device(_code(*key), seeds, channel)
    return _dev[k]


@pytest.mark.parametrize("key", CODES, ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("channel", ["awgn", "bsc"])
def test_draw_blocks_device_against_numpy(lib_gpu, key, channel):
    from sparc_ldpc_amd import ldpc_mc
    code = _code(*key)
    K = ldpc_mc.info_bits(code, channel)
    assert K == (code.K if channel == "awgn" and key[0] != "2_7_12_good" else 0)
    u0, w0 = ldpc_mc._draw_blocks(SEEDS, K, code.N, channel)
    u, w = _device_blocks(key, SEEDS, channel)
    assert w.shape == w0.shape == (len(SEEDS), code.N)
    if K:
        assert u.dtype == np.uint8
        np.testing.assert_array_equal(u, u0)
    else:
        assert u is None and u0 is None
    if channel == "bsc":
        np.testing.assert_array_equal(w, w0)
        return
    zero = w0 == 0
    ratio = np.abs(w - w0)[~zero] / np.abs(w0[~zero])
    differ = int((w != w0).sum())
    print(f"{key}: {differ} of {w.size} values differ ({100.0 * differ / w.size:.3f} %), "
          f"largest ratio {ratio.max() * 2.0 ** 52:.3f} * 2**-52")
    assert np.all(w[zero] == 0) and np.all(np.isfinite(w))
    assert ratio.max() <= BAR


@pytest.mark.parametrize("key", CODES[:2], ids=lambda k: "-".join(map(str, k)))
def test_mc_ldpc_device_draws_awgn(lib_gpu, key):
    """Per-block errors and iteration counts of mc_ldpc(draws="device") equal
    mc_blocks on the arrays draw_blocks_device returned, whatever the batch."""
    from sparc_ldpc_amd import ldpc_mc
    code = _code(*key)
    sigma = SIGMA[key]
    u, w = _device_blocks(key, MC_SEEDS, "awgn")
    be0, it0 = code.mc_blocks(u, w, sigma, "awgn", 16)
    print(f"{key}: failed={int((be0 > 0).sum())} clean={int((be0 == 0).sum())}")
    assert (be0 > 0).any() and (be0 == 0).any(), "the case must hold both clean and failed blocks"
    for batch in (16, 7, 64):
        be, it = ldpc_mc.mc_ldpc(code, sigma, MC_SEEDS, batch=batch, draws="device")
        assert be.dtype == np.int64 and it.dtype == np.int64
        np.testing.assert_array_equal(be, be0, err_msg=f"batch {batch}")
        np.testing.assert_array_equal(it, it0, err_msg=f"batch {batch}")


@pytest.mark.parametrize("key", CODES, ids=lambda k: "-".join(map(str, k)))
def test_mc_ldpc_device_draws_bsc_equals_host_draws(lib_gpu, key):
    """The BSC's draws are exact, so the whole result is the host-draw path's."""
    from sparc_ldpc_amd import ldpc_mc
    code = _code(*key)
    be0, it0 = ldpc_mc.mc_ldpc(code, 0.03, MC_SEEDS, channel="bsc", batch=16)
    for batch in (16, 7, 64):
        be, it = ldpc_mc.mc_ldpc(code, 0.03, MC_SEEDS, channel="bsc", batch=batch, draws="device")
        np.testing.assert_array_equal(be, be0, err_msg=f"batch {batch}")
        np.testing.assert_array_equal(it, it0, err_msg=f"batch {batch}")


def test_sim_ldpc_mc_device_draws(lib_gpu):
    """sim_ldpc_mc(draws="device") applies the stopping rule to the device-drawn
    blocks' outputs, whatever the batch; the all-zero branch (K = 0) runs too."""
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_mc
    key = ("802.16", "5/6", 8)
    code = _code(*key)
    be, it = ldpc_mc.mc_ldpc(code, 0.56, range(100, 164), batch=64, draws="device")
    nbit = nerr = nblocks = nit = 0
    while nerr < 5:  # sparc_ldpc.py:1097-1122 over the per-block outputs
        nbit += int(be[nblocks])
        nerr += 1 if be[nblocks] else 0
        nit += int(it[nblocks])
        nblocks += 1
    want = dict(ber=nbit / (nblocks * code.N), blocks=nblocks, block_errors=nerr, bit_errors=nbit, nit_total=nit)
    lp = sp.LDPCParams(*key)
    for batch in (7, 16):
        tm = {}
        got = sp.sim_ldpc_mc(lp, 0.56, MIN_ERRORS=5, MAX_BLOCKS=1000, seed0=100, batch=batch, draws="device",
                             timings=tm)
        assert got == want, batch
        assert tm["device_ms"] > 0
    zero_code = _code(*CODES[2])
    u, w = _device_blocks(CODES[2], MC_SEEDS, "awgn")
    be0, it0 = zero_code.mc_blocks(None, w, 0.8, "awgn", 16)
    be1, it1 = ldpc_mc.mc_ldpc(zero_code, 0.8, MC_SEEDS, batch=16, draws="device")
    np.testing.assert_array_equal(be1, be0)
    np.testing.assert_array_equal(it1, it0)
