"""GPU: the device-side LDPC Monte-Carlo (csrc/ldpc_mc.hip) against the host
pipeline it replaces — _draw_blocks -> encode_batch -> the LLR expression of
the seed contract -> decode_batch -> the NumPy error count: the encoder alone,
per-block bit errors and iteration counts, batch independence, the stopping
rule of sim_ldpc_mc and waterfall's opt-in BPSK column."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = list(range(100, 137))  # 37 blocks: batch 16 gives two full batches and a partial one

# (standard, rate, z, ptype, channel, a, seeds, batch, failed blocks by the NumPy oracle)
CASES = {
    "802.16-1/2-z24": ("802.16", "1/2", 24, "A", "awgn", 0.85, SEEDS, 16, 12),
    "802.11n-5/6-z27": ("802.11n", "5/6", 27, "A", "awgn", 0.56, SEEDS, 16, 24),
    "802.16-2/3B-z3": ("802.16", "2/3", 3, "B", "awgn", 0.75, SEEDS, 16, 26),
    "802.16-3/4B-z100": ("802.16", "3/4", 100, "B", "awgn", 0.62, SEEDS, 16, 4),
    "802.16-5/6-z192": ("802.16", "5/6", 192, "A", "awgn", 0.56, list(range(100, 108)), 8, 5),  # the benched shape
    "bsc-802.16-1/2-z24": ("802.16", "1/2", 24, "A", "bsc", 0.075, SEEDS, 16, 12),
}

_codes, _host = {}, {}


def _code(std, rate, z, ptype):
    from sparc_ldpc_amd import ldpc
    key = (std, rate, z, ptype)
    if key not in _codes:
        _codes[key] = ldpc.code(std, rate, z, ptype)
    return _codes[key]


def _host_pipeline(name):
    """Per-block (bit_errors, iters) of a case by the host pipeline; computed once."""
    if name in _host:
        return _host[name]
    from sparc_ldpc_amd import ldpc_mc
    std, rate, z, ptype, channel, a, seeds = CASES[name][:7]
    code = _code(std, rate, z, ptype)
    u, w = ldpc_mc._draw_blocks(seeds, ldpc_mc.info_bits(code, channel), code.N, channel)
    if channel == "awgn":
        x = code.encode_batch(u)
        sigma = float(a)
        ch = (2.0 / sigma ** 2) * ((1.0 - 2.0 * x) + sigma * w)
    else:
        x = np.zeros((len(seeds), code.N), dtype=np.int64)
        p = float(a)
        llr = math.log((1 - p) / p)
        ch = np.where(w < p, -llr, llr)
    app, it = code.decode_batch(ch, "sumprod2")
    be = ((app < 0.0) != x).sum(axis=1).astype(np.int64)
    _host[name] = (be, it)
    return _host[name]


def test_encode_device_equals_encode_batch(lib_gpu):
    from sparc_ldpc_amd import ldpc, ldpc_awgn
    cases = list(ldpc_awgn.sim_param)
    cases += [("802.16", rate, z, "A") for z in (8, 100, 192) for rate in ("1/2", "5/6")]
    assert {c[2] for c in cases} >= {3, 27, 100}  # narrower than a wavefront; not powers of two
    rs = np.random.RandomState(11)
    for std, rate, z, ptype in cases:
        code = ldpc.code(std, rate, z, ptype)
        U = rs.randint(0, 2, (3, code.K))
        X = code.encode_device(U)
        assert X.dtype == np.uint8 and X.shape == (3, code.N)
        assert np.array_equal(X, code.encode_batch(U)), (std, rate, z, ptype)


@pytest.mark.parametrize("name", list(CASES))
def test_mc_ldpc_equals_host_pipeline(lib_gpu, name):
    from sparc_ldpc_amd import ldpc_mc
    std, rate, z, ptype, channel, a, seeds, batch, nfailed = CASES[name]
    be0, it0 = _host_pipeline(name)
    failed, clean = int((be0 > 0).sum()), int((be0 == 0).sum())
    print(f"{name}: host pipeline failed={failed} clean={clean} iters={it0.tolist()}")
    assert failed > 0 and clean > 0, "the case must hold both clean and failed blocks"
    assert failed == nfailed
    if name == "802.16-2/3B-z3":
        # a block that converges (before max_iter) to a wrong codeword
        assert np.any((be0 > 0) & (it0 < 200))
    be, it = ldpc_mc.mc_ldpc(_code(std, rate, z, ptype), a, seeds, channel=channel, batch=batch)
    assert be.dtype == np.int64 and it.dtype == np.int64
    assert np.array_equal(it, it0)
    assert np.array_equal(be, be0)


def test_mc_ldpc_batch_independence(lib_gpu):
    from sparc_ldpc_amd import ldpc_mc
    code = _code("802.16", "1/2", 24, "A")
    be0, it0 = _host_pipeline("802.16-1/2-z24")
    for batch in (7, 16, 64):
        be, it = ldpc_mc.mc_ldpc(code, 0.85, SEEDS, batch=batch)
        assert np.array_equal(be, be0) and np.array_equal(it, it0), batch


@pytest.mark.parametrize("min_errors,max_blocks", [(5, 1000), (100, 10)])
def test_sim_ldpc_mc_stopping_rule(lib_gpu, min_errors, max_blocks):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_mc
    code = _code("802.16", "1/2", 24, "A")
    be, it = ldpc_mc.mc_ldpc(code, 0.85, range(100, 164), batch=64)
    nbit = nerr = nblocks = nit = 0
    while nerr < min_errors:  # sparc_ldpc.py:1097-1122 over the per-block outputs
        nbit += int(be[nblocks])
        nerr += 1 if be[nblocks] else 0
        nit += int(it[nblocks])
        nblocks += 1
        if nblocks >= max_blocks:
            break
    want = dict(ber=nbit / (nblocks * code.N), blocks=nblocks, block_errors=nerr, bit_errors=nbit, nit_total=nit)
    lp = sp.LDPCParams("802.16", "1/2", 24)
    for batch in (7, 16):
        got = sp.sim_ldpc_mc(lp, 0.85, MIN_ERRORS=min_errors, MAX_BLOCKS=max_blocks, seed0=100, batch=batch)
        assert got == want, batch


def test_waterfall_bpsk_mc(lib_gpu):
    """The opt-in BPSK column at the small joint shape of test_batched_joint_equals_per_rep."""
    import sparc_ldpc_amd as sp
    spp = sp.SPARCParams(64, 16, 0.93, 4.0, 1.0, 30)
    lp = sp.LDPCParams("802.16", "5/6", None)
    kw = dict(init="soft", MIN_ERRORS=3, MAX_BLOCKS=8, bpsk=True, sections=48, batch=4, seed0=40, ebno_dbs=[4.0],
              precision="fp64")
    today = sp.waterfall(spp, lp, **kw)
    off = sp.waterfall(spp, lp, bpsk_mc=False, **kw)
    on = sp.waterfall(spp, lp, bpsk_mc=True, **kw)
    assert off == today
    # today's column: sim_ldpc on the z = 8 code, seeded base + 7_000_000
    sigma_bpsk = np.sqrt((1 / 10 ** (4.0 / 20)) / 2)
    ldp = sp.LDPCParams("802.16", "5/6", 8)
    assert off[0]["BER_bpsk"] == sp.sim_ldpc(ldp, sigma_bpsk, 3, 8, seed=40 + 7_000_000)
    assert np.isfinite(on[0]["BER_bpsk"]) and 0.0 <= on[0]["BER_bpsk"] <= 1.0
    assert on[0]["BER_bpsk"] == sp.sim_ldpc_mc(ldp, float(sigma_bpsk), 3, 8, seed0=40 + 7_000_000)["ber"]
    for k in on[0]:
        if k != "BER_bpsk":
            assert on[0][k] == off[0][k], k
