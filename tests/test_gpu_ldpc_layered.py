"""GPU: the layered belief-propagation kernel k_bpl (every instance of
DESIGN.md §10's layered table) against the NumPy reference of the schedule
(tests/ldpc_layered_ref.py) at fixed sweep counts: decodes cut at max_iter = k
through lb_decode (host pointers) and through lb_stage + lb_run + lb_fetch, on
words that stop after 0, 1, 3 and >= 6 sweeps, never converge, belong to no
codeword, carry erased bits of either sign of zero, or are saturated.

Bars: sweep counts exact; layered_minsum app bit-equal, sign bit included (the
kernel and the reference perform the same IEEE operations in the same order,
no transcendental); layered_sumprod2 within the suite's TOL["sumprod2"]
(rtol = atol).  The words' seeds were chosen from the reference alone
(tests/ldpc_layered_cases.py), and what they must satisfy is asserted here
from the reference alone."""
import ctypes as ct

import numpy as np
import pytest

import ldpc_layered_cases as llc
import ldpc_layered_ref as lr
from test_gpu_ldpc import TOL

pytestmark = pytest.mark.gpu

_IP = ct.POINTER(ct.c_int)
_DP = ct.POINTER(ct.c_double)


@pytest.fixture(scope="module")
def bp():
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible: -m gpu tests need an MI355X"
    return ldpc


class _Worst:
    """Largest deviation from the reference seen in a test, relative to max(1, |app|) (printed: DESIGN.md §10)."""

    def __init__(self):
        self.dev = 0.0

    def compare(self, algo, app, it, rapp, rit, what):
        assert np.array_equal(it, rit), (what, it, rit)
        if algo == "minsum":
            assert np.array_equal(app, rapp), (what, np.argwhere(app != rapp)[:4])
            assert np.array_equal(np.signbit(app), np.signbit(rapp)), what
            return
        with np.errstate(invalid="ignore"):
            d = np.abs(app - rapp) / np.maximum(1.0, np.abs(rapp))
        self.dev = max(self.dev, float(np.max(np.where(app == rapp, 0.0, d))))
        np.testing.assert_allclose(app, rapp, rtol=TOL["sumprod2"], atol=TOL["sumprod2"], err_msg=str(what))


def _staged(bp, c, ch, dectype, k):
    B = ch.shape[0]
    c.device_buffers(B)
    lib = bp.load_bp_library()
    assert lib.lb_stage(c._context(), B, np.ascontiguousarray(ch).ctypes.data_as(_DP)) == 0
    c.run_buffers(B, dectype, max_iter=k)
    return c.fetch_buffers(B)


@pytest.mark.parametrize("algo", llc.ALGOS)
@pytest.mark.parametrize("cell", list(llc.CELLS))
def test_truncated_decodes_against_reference(bp, cell, algo):
    ref = llc.reference(cell, algo)
    ref.check_preconditions(cell, algo)
    W = len(ref.CH)
    c = llc.make_code(cell)
    dectype = "layered_" + algo
    assert c.layer_info()["nlayers"] == 0  # set on first layered use
    worst = _Worst()
    call = 0
    for k in llc.KS:
        for how in ("host", "staged"):
            # another order and another number of words every call
            idx = np.roll(np.arange(W), call)[:W - call % 3] if W > 2 else np.arange(W)[::1 - 2 * (call % 2)]
            call += 1
            if how == "host":
                app, it = c.decode_batch(ref.CH[idx], dectype, max_iter=k)
            else:
                app, it = _staged(bp, c, ref.CH[idx], dectype, k)
            worst.compare(algo, app, it, *ref.at(k, idx), (how, k, idx.tolist()))
    info = c.layer_info()
    lds, max_layer, threads = llc.CELLS[cell][1]
    assert info == dict(nlayers=c.Nc // c.z, max_layer=max_layer, lds_messages=lds, threads=threads)
    assert max_layer == c.z
    print(f"\nlayered {cell} {algo}: sweeps={ref.its.tolist()} worst deviation {worst.dev:.3e}")


@pytest.mark.parametrize("algo", llc.ALGOS)
def test_max_iter_zero_returns_the_channel(bp, algo):
    for cell in ("16_1/2_z24", "16_5/6_z300"):
        ref = llc.reference(cell, algo)
        c = llc.make_code(cell)
        c.decode_batch(ref.CH, "layered_" + algo, max_iter=2)  # the buffers hold something else
        for app, it in (c.decode_batch(ref.CH, "layered_" + algo, max_iter=0),
                        _staged(bp, c, ref.CH, "layered_" + algo, 0)):
            assert np.array_equal(app, ref.CH) and np.array_equal(np.signbit(app), np.signbit(ref.CH))
            assert it.shape == (len(ref.CH),) and not it.any()
        with pytest.raises(AssertionError):
            c.decode_batch(ref.CH, "layered_" + algo, max_iter=-1)


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("cell", ["16_1/2_z24", "16_5/6_z24", "syn_dc32"])
def test_messages_kept_out_of_lds(bp, monkeypatch, cell, lds):
    """LDPC_BP_LAYERED_LDS: the HBM instances of the small cells' kernels, same bars."""
    monkeypatch.setenv("LDPC_BP_LAYERED_LDS", str(lds))
    worst = _Worst()
    for algo in llc.ALGOS:
        ref = llc.reference(cell, algo)
        c = llc.make_code(cell)
        for k in (3, 12):
            app, it = c.decode_batch(ref.CH, "layered_" + algo, max_iter=k)
            assert c.layer_info()["lds_messages"] == lds
            worst.compare(algo, app, it, *ref.at(k), (lds, k))
    print(f"\nlayered {cell} lds_messages={lds}: worst deviation {worst.dev:.3e}")


@pytest.mark.parametrize("threads", [64, 128, 1024])
@pytest.mark.parametrize("cell", ["16_1/2_z96", "16_5/6_z24"])
def test_thread_counts(bp, monkeypatch, cell, threads):
    """LDPC_BP_LAYERED_THREADS: a layer's checks and edges strided over fewer threads than there are
    (802.16 1/2 z=96: 96 checks and 672 edges over 64 and 128), and more threads than edges."""
    monkeypatch.setenv("LDPC_BP_LAYERED_THREADS", str(threads))
    worst = _Worst()
    for algo in llc.ALGOS:
        ref = llc.reference(cell, algo)
        c = llc.make_code(cell)
        app, it = c.decode_batch(ref.CH, "layered_" + algo, max_iter=12)
        assert c.layer_info()["threads"] == min(threads, 768 if cell == "16_5/6_z24" else 1024)
        worst.compare(algo, app, it, *ref.at(12), threads)
    print(f"\nlayered {cell} threads={threads}: worst deviation {worst.dev:.3e}")


@pytest.mark.parametrize("algo", llc.ALGOS)
def test_more_words_than_cus_at_one_word_per_cu(bp, algo):
    """802.16 5/6 z=192: the 156 KB image holds one word per CU, so in a launch of more words than
    CUs (256) workgroups follow each other on a CU.  The cell's two words, 300 copies each in a
    shuffled order: the same bars, and the same bits as the two-word launch."""
    cell = "16_5/6_z192"
    ref = llc.reference(cell, algo)
    c = llc.make_code(cell)
    idx = np.random.RandomState(7).permutation(np.repeat(np.arange(2), 300))
    worst = _Worst()
    for k in (3, 12):
        small = c.decode_batch(ref.CH, "layered_" + algo, max_iter=k)
        for app, it in (c.decode_batch(ref.CH[idx], "layered_" + algo, max_iter=k),
                        _staged(bp, c, ref.CH[idx], "layered_" + algo, k)):
            worst.compare(algo, app, it, *ref.at(k, idx), k)
            assert np.array_equal(app, small[0][idx]) and np.array_equal(it, small[1][idx])
    print(f"\nlayered {cell} {algo} 600 words: worst deviation {worst.dev:.3e}")


def _raw_set_layers(bp, c, fc):
    fc = np.ascontiguousarray(fc, dtype=np.intc)
    lib = bp.load_bp_library()
    rc = lib.lb_set_layers(c._context(), len(fc) - 1, fc.ctypes.data_as(_IP))
    return rc, lib.lb_last_error().decode()


def test_set_layers_rejections_leave_the_context_usable(bp):
    cell = "16_1/2_z24"
    ref = llc.reference(cell, "sumprod2")
    c = llc.make_code(cell)
    fc = lr.code_layers(c)
    flood0 = c.decode_batch(ref.CH, "sumprod2", max_iter=12)
    lay0 = c.decode_batch(ref.CH, "layered_sumprod2", max_iter=12)
    want_info = c.layer_info()
    merged = np.delete(fc, 1)  # protograph rows 0 and 1 in one layer: they share columns
    v_twice = None
    vo = lr.var_of(c.vdeg, c.intrlv)[:np.cumsum(c.cdeg)[2 * c.z - 1]]
    seen = set()
    for v in vo:  # the first variable the library meets twice, walking the edges in order
        if int(v) in seen:
            v_twice = int(v)
            break
        seen.add(int(v))
    bad = {
        "non-increasing": np.concatenate([fc[:3], fc[2:]]),
        "decreasing": np.concatenate([fc[:2], [fc[3], fc[2]], fc[4:]]),
        "last entry short of Nc": fc[:-1],
        "last entry past Nc": np.concatenate([fc[:-1], [c.Nc + 1]]),
        "does not start at 0": np.concatenate([[1], fc[1:]]),
        "two rows merged": merged,
    }
    for what, layers in bad.items():
        rc, msg = _raw_set_layers(bp, c, layers)
        assert rc == -4, (what, rc, msg)  # LB_ERR_GRAPH
        if what == "two rows merged":
            assert "layer 0" in msg and f"variable {v_twice} " in msg, msg
        with pytest.raises(bp.LdpcBpError) as e:
            c.set_layers(layers)
        assert e.value.code == -4
        # the context is as it was: the same layers, the same results, flooding and layered
        assert c.layer_info() == want_info
        app, it = c.decode_batch(ref.CH, "sumprod2", max_iter=12)
        assert np.array_equal(app, flood0[0]) and np.array_equal(it, flood0[1]), what
    app, it = c.decode_batch(ref.CH, "layered_sumprod2", max_iter=12)
    assert np.array_equal(app, lay0[0]) and np.array_equal(it, lay0[1])
    # a finer layering is accepted and decodes (to a codeword, by its own route)
    split = np.unique(np.concatenate([fc, fc[:-1] + c.z // 2]))
    c.set_layers(split)
    assert c.layer_info()["nlayers"] == 2 * (len(fc) - 1) and c.layer_info()["max_layer"] == c.z // 2
    rapp, rit = zip(*[lr.decode(ch, c.vdeg, c.cdeg, c.intrlv, split, max_it=12) for ch in ref.CH])
    app, it = c.decode_batch(ref.CH, "layered_sumprod2", max_iter=12)
    assert np.array_equal(it, rit)
    np.testing.assert_allclose(app, np.array(rapp), rtol=TOL["sumprod2"], atol=TOL["sumprod2"])


def test_layered_decode_without_layers_is_an_argument_error(bp):
    """Through the raw ABI on a fresh context: code.decode_batch would set the layers first."""
    c = llc.make_code("16_1/2_z24")
    lib = bp.load_bp_library()
    ch = np.ascontiguousarray(llc.reference("16_1/2_z24", "sumprod2").CH[:2])
    app = np.empty_like(ch)
    it = np.empty(2, dtype=np.intc)
    for algo in (bp.LB_LAYERED_SUMPROD2, bp.LB_LAYERED_MINSUM):
        for max_iter in (0, 5):
            rc = lib.lb_decode(c._context(), 2, ch.ctypes.data_as(_DP), app.ctypes.data_as(_DP), it.ctypes.data_as(_IP),
                               algo, 0.7, max_iter)
            assert rc == -1 and b"layers" in lib.lb_last_error()
        assert lib.lb_stage(c._context(), 2, ch.ctypes.data_as(_DP)) == 0
        assert lib.lb_run(c._context(), 2, algo, 0.7, 5) == -1
    assert lib.lb_decode(c._context(), 2, ch.ctypes.data_as(_DP), app.ctypes.data_as(_DP), it.ctypes.data_as(_IP),
                         5, 0.7, 5) == -1  # past the last decoder type
    out = (ct.c_int64 * 4)()
    assert lib.lb_layer_info(c._context(), out) == 0 and list(out)[:2] == [0, 0]
    # and the names: decode keeps the reference's three
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        c.decode(ch[0], "layered_sumprod2")
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        c.decode_batch(ch, "layered_sumprod")


@pytest.mark.parametrize("cell", ["16_1/2_z24", "16_5/6_z24", "16_5/6_z300"])
def test_flooding_decodes_are_untouched_by_layered_ones(bp, cell):
    """The same flooding decode before and after layered decodes on one context (tail on: the message
    slices in HBM are shared), host- and device-sized: identical bits."""
    ref = llc.reference(cell, "sumprod2")
    c = llc.make_code(cell)
    before = [c.decode_batch(ref.CH, a, max_iter=12) for a in ("sumprod2", "minsum")]
    staged0 = _staged(bp, c, ref.CH, "sumprod2", 12)
    info0 = c.info()
    for a in llc.ALGOS:
        c.decode_batch(ref.CH, "layered_" + a, max_iter=12)
        _staged(bp, c, ref.CH[::-1], "layered_" + a, 3)
    assert c.info() == info0
    after = [c.decode_batch(ref.CH, a, max_iter=12) for a in ("sumprod2", "minsum")]
    for (a0, i0), (a1, i1) in zip(before + [staged0], after + [_staged(bp, c, ref.CH, "sumprod2", 12)]):
        assert np.array_equal(a0, a1) and np.array_equal(np.signbit(a0), np.signbit(a1)) and np.array_equal(i0, i1)


def test_mc_blocks_layered_equal_decode_batch(bp):
    from sparc_ldpc_amd import ldpc_mc
    c = bp.code("802.16", "1/2", 24)
    seeds = np.arange(200, 212)
    sigma = 0.8

    def want(u, w, dectype):
        x = c.encode_batch(u)
        ch = (2.0 / sigma ** 2) * ((1.0 - 2.0 * x) + sigma * w)
        app, it = c.decode_batch(ch, dectype)
        return ((app < 0.0) != x).sum(axis=1), it

    u, w = ldpc_mc._draw_blocks(seeds, c.K, c.N, "awgn")
    ud, wd = ldpc_mc.draw_blocks_device(c, seeds)
    for dectype in ("layered_sumprod2", "layered_minsum"):
        be0, it0 = want(u, w, dectype)
        assert it0.min() >= 1 and len(set(it0.tolist())) > 2
        be, it = c.mc_blocks(u, w, sigma, dectype=dectype, batch=5)
        assert np.array_equal(be, be0) and np.array_equal(it, it0)
        be0, it0 = want(ud, wd, dectype)
        be, it = c.mc_blocks_seeds(seeds, sigma, dectype=dectype, batch=5)
        assert np.array_equal(be, be0) and np.array_equal(it, it0)
        be, it = ldpc_mc.mc_ldpc(c, sigma, seeds, batch=7, dectype=dectype, draws="device")
        assert np.array_equal(be, be0) and np.array_equal(it, it0)
    # fewer sweeps than flooding iterations on the same blocks
    assert c.mc_blocks(u, w, sigma, dectype="layered_sumprod2")[1].sum() < c.mc_blocks(u, w, sigma)[1].sum()


def test_sim_ldpc_mc_layered(bp):
    import sparc_ldpc_amd as sp
    lp = sp.LDPCParams("802.16", "1/2", 24)
    never = 10 ** 9
    kw = dict(MIN_ERRORS=never, MAX_BLOCKS=64, batch=32)
    flood = sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, **kw)
    assert flood == sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, dectype="sumprod2", **kw)
    for draws in ("host", "device"):
        lay = sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, dectype="layered_sumprod2", draws=draws, **kw)
        assert lay["blocks"] == flood["blocks"] == 64
        assert lay["bit_errors"] <= flood["bit_errors"]
        assert lay["block_errors"] <= flood["block_errors"]
        assert 0 < lay["nit_total"] < flood["nit_total"]  # sweeps against iterations
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, dectype="layered", **kw)


def test_awgn_and_bsc_sweeps_take_a_decoder_type(bp):
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc
    # 6 dB above the AWGN rate's SNR (sigma = 0.78): most blocks decode, in fewer sweeps than iterations
    kw = dict(N_MEASUREMENTS=2, C_AWGN_OFFSET=6.0, MIN_ERRORS=3, MAX_BLOCKS=24, batch=8)
    flood = ldpc_awgn.sim("802.16", "1/2", 24, **kw)
    lay = ldpc_awgn.sim("802.16", "1/2", 24, dectype="layered_sumprod2", **kw)
    assert len(lay) == len(flood) == 2 and lay[0][:4] == flood[0][:4]
    assert lay[0][8] / lay[0][4] < flood[0][8] / flood[0][4]  # nit_total per block: sweeps against iterations
    res, parray = ldpc_bsc.sim("802.16", "1/2", 24, repeats=6, dectype="layered_minsum")
    assert len(res) == len(parray) == 10 and res[-1] == 0.0  # p = 0.001: no bit error left
    for sim in (ldpc_awgn.sim, ldpc_bsc.sim):
        with pytest.raises(NameError, match="Decoder type unknonwn"):
            sim("802.16", "1/2", 24, dectype="nope")
    with pytest.raises(TypeError):
        ldpc_bsc.sim("802.16", "1/2", 24, "A", "layered_sumprod2")  # keyword-only
