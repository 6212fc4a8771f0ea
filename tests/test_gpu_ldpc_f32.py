"""GPU: the binary32 layered belief-propagation kernel k_bpl32 (LB_F32; every
instance and layout of DESIGN.md §10's binary32 table) against its NumPy
statement (tests/ldpc_f32_ref.py) at fixed sweep counts: decodes cut at
max_iter = k through lb_decode (host pointers) and through lb_stage + lb_run +
lb_fetch, on words that stop after 0, 1, 3 and >= 6 sweeps, never converge,
belong to no codeword, carry erased bits of either sign of zero, are saturated,
or hold +-DBL_MAX and +-inf (the clamp on load).

Bars: sweep counts exact; layered_minsum_f32 app bit-equal, sign bit included
(the kernel and the statement perform the same IEEE binary32 operations in the
same order); layered_sumprod2_f32 within B = 16 P, rtol = atol, P being how far
the statement itself moves between NumPy's float32 exp / log and a correctly
rounded log(1 + exp(-x)) (tests/ldpc_f32_cases.py).  The words' seeds were
chosen from the statement alone, and what they must satisfy is asserted here
from the statement alone."""
import ctypes as ct

import numpy as np
import pytest

import ldpc_f32_cases as fc
import ldpc_layered_cases as llc

pytestmark = pytest.mark.gpu

_IP = ct.POINTER(ct.c_int)
_DP = ct.POINTER(ct.c_double)
LB_F32 = 0x100


@pytest.fixture(scope="module")
def bp():
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible: -m gpu tests need an MI355X"
    return ldpc


class _Worst:
    """Largest deviation from the statement seen in a test, relative to max(1, |app|) (printed: DESIGN.md §10)."""

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
        np.testing.assert_allclose(app, rapp, rtol=fc.B, atol=fc.B, err_msg=str(what))


def _dectype(algo):
    return "layered_" + algo + "_f32"


def _staged(bp, c, ch, dectype, k):
    B = ch.shape[0]
    c.device_buffers(B)
    lib = bp.load_bp_library()
    assert lib.lb_stage(c._context(), B, np.ascontiguousarray(ch).ctypes.data_as(_DP)) == 0
    c.run_buffers(B, dectype, max_iter=k)
    return c.fetch_buffers(B)


def _check_info(c, cell, algo, lds=None, threads=None):
    want_lds, max_layer, want_threads, lds_bytes, resident = fc.CELLS[cell]
    info = c.layer_info("f32")
    assert info["nlayers"] == c.Nc // c.z and info["max_layer"] == max_layer == c.z
    assert info["message_bytes"] == 4
    if lds is None and threads is None:
        assert (info["lds_messages"], info["threads"], info["lds_bytes"]) == (want_lds, want_threads, lds_bytes), info
        assert info["resident" if algo == "sumprod2" else "resident_minsum"] == resident, info
    return info


@pytest.mark.parametrize("algo", fc.ALGOS)
@pytest.mark.parametrize("cell", list(fc.CELLS))
def test_truncated_decodes_against_statement(bp, cell, algo):
    ref = fc.reference(cell, algo)
    ref.check_preconditions()
    W = len(ref.CH)
    c = fc.make_code(cell)
    dectype = _dectype(algo)
    assert c.layer_info("f32")["nlayers"] == 0 and c.layer_info("f32")["resident"] == 0  # set on first layered use
    worst = _Worst()
    call = 0
    for k in fc.KS:
        for how in ("host", "staged"):
            # another order and another number of words every call
            idx = np.roll(np.arange(W), call)[:W - call % 3] if W > 2 else np.arange(W)[::1 - 2 * (call % 2)]
            call += 1
            if how == "host":
                app, it = c.decode_batch(ref.CH[idx], dectype, max_iter=k)
            else:
                app, it = _staged(bp, c, ref.CH[idx], dectype, k)
            worst.compare(algo, app, it, *ref.at(k, idx), (how, k, idx.tolist()))
    info = _check_info(c, cell, algo)
    # the binary64 figures are what they were
    lds, max_layer, threads = llc.CELLS[cell][1]
    assert c.layer_info() == dict(nlayers=c.Nc // c.z, max_layer=max_layer, lds_messages=lds, threads=threads)
    print(f"\nf32 layered {cell} {algo}: sweeps={ref.its.tolist()} worst deviation {worst.dev:.3e} "
          f"(P_cell {fc.P_CELL[cell]:.3e}, B {fc.B:.3e}) {info}")


def test_binary32_layout_uses_the_element_size(bp):
    """802.16 5/6 z=300: 31200 messages and LLRs are 250 KB in binary64 (r in HBM) and 125 KB in binary32 (LDS);
    5/6 z=192: two binary32 workgroups share a CU where one binary64 workgroup fills it."""
    c = fc.make_code("16_5/6_z300")
    c.set_layers(np.arange(0, c.Nc + 1, c.z))
    assert c.layer_info()["lds_messages"] == 1 and c.layer_info("f32")["lds_messages"] == 2
    c = fc.make_code("16_5/6_z192")
    c.set_layers(np.arange(0, c.Nc + 1, c.z))
    info = c.layer_info("f32")
    assert info["lds_bytes"] == 4 * (c.Nv + c.Nmsg) == 79872 and info["threads"] == 768
    assert info["resident"] == 2 and info["resident_minsum"] == 2
    lib = bp.load_bp_library()
    out = (ct.c_int64 * 8)()
    assert lib.lb_layer_info_ex(c._context(), 0, out) == 0
    assert list(out)[:5] == [4, 192, 2, 768, 8 * (c.Nv + c.Nmsg)] and out[5] == 1 and out[6] == 1 and out[7] == 8
    assert lib.lb_layer_info_ex(c._context(), 2, out) == -1


@pytest.mark.parametrize("algo", fc.ALGOS)
def test_max_iter_zero_returns_the_channel_unclamped(bp, algo):
    for cell in ("16_1/2_z24", "16_5/6_z300"):
        ref = fc.reference(cell, algo)
        c = fc.make_code(cell)
        c.decode_batch(ref.CH, _dectype(algo), max_iter=2)  # the buffers hold something else
        for app, it in (c.decode_batch(ref.CH, _dectype(algo), max_iter=0),
                        _staged(bp, c, ref.CH, _dectype(algo), 0)):
            assert np.array_equal(app, ref.CH) and np.array_equal(np.signbit(app), np.signbit(ref.CH))
            assert it.shape == (len(ref.CH),) and not it.any()
        with pytest.raises(AssertionError):
            c.decode_batch(ref.CH, _dectype(algo), max_iter=-1)


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("cell", ["16_1/2_z24", "16_5/6_z24", "syn_dc32"])
def test_messages_kept_out_of_lds(bp, monkeypatch, cell, lds):
    """LDPC_BP_LAYERED_LDS: the HBM instances of each DCMAX / DCFIX (r, and with 0 also app, as floats in
    the context's message slices), same bars."""
    monkeypatch.setenv("LDPC_BP_LAYERED_LDS", str(lds))
    worst = _Worst()
    for algo in fc.ALGOS:
        ref = fc.reference(cell, algo)
        c = fc.make_code(cell)
        for k in (3, 12):
            app, it = c.decode_batch(ref.CH, _dectype(algo), max_iter=k)
            info = _check_info(c, cell, algo, lds=lds)
            assert info["lds_messages"] == lds and info["lds_bytes"] == (4 * c.Nv if lds else 0)
            worst.compare(algo, app, it, *ref.at(k), (lds, k))
    print(f"\nf32 layered {cell} lds_messages={lds}: worst deviation {worst.dev:.3e}")


@pytest.mark.parametrize("threads", [64, 128])
def test_thread_counts(bp, monkeypatch, threads):
    """LDPC_BP_LAYERED_THREADS at 802.16 1/2 z=96: a layer's 96 checks and 672 edges strided over 64 and 128 threads."""
    cell = "16_1/2_z96"
    monkeypatch.setenv("LDPC_BP_LAYERED_THREADS", str(threads))
    worst = _Worst()
    for algo in fc.ALGOS:
        ref = fc.reference(cell, algo)
        c = fc.make_code(cell)
        app, it = c.decode_batch(ref.CH, _dectype(algo), max_iter=12)
        assert _check_info(c, cell, algo, threads=threads)["threads"] == threads
        worst.compare(algo, app, it, *ref.at(12), threads)
    print(f"\nf32 layered {cell} threads={threads}: worst deviation {worst.dev:.3e}")


@pytest.mark.parametrize("algo", fc.ALGOS)
def test_more_words_than_slots_at_two_words_per_cu(bp, algo):
    """802.16 5/6 z=192: the 78 KB image lets two words share a CU (512 slots on 256 CUs).  The cell's two
    words, 300 copies each in a shuffled order: more workgroups than slots, the same bars, and the same
    bits as the two-word launch."""
    cell = "16_5/6_z192"
    ref = fc.reference(cell, algo)
    c = fc.make_code(cell)
    idx = np.random.RandomState(7).permutation(np.repeat(np.arange(2), 300))
    worst = _Worst()
    for k in (3, 12):
        small = c.decode_batch(ref.CH, _dectype(algo), max_iter=k)
        for app, it in (c.decode_batch(ref.CH[idx], _dectype(algo), max_iter=k),
                        _staged(bp, c, ref.CH[idx], _dectype(algo), k)):
            worst.compare(algo, app, it, *ref.at(k, idx), k)
            assert np.array_equal(app, small[0][idx]) and np.array_equal(it, small[1][idx])
    print(f"\nf32 layered {cell} {algo} 600 words: worst deviation {worst.dev:.3e}")


def _raw_decode(lib, c, ch, algo, max_iter):
    app = np.full_like(ch, 7.0)
    it = np.full(len(ch), -3, dtype=np.intc)
    rc = lib.lb_decode(c._context(), len(ch), ch.ctypes.data_as(_DP), app.ctypes.data_as(_DP), it.ctypes.data_as(_IP),
                       algo, 0.7, max_iter)
    return rc, lib.lb_last_error().decode(), app, it


def test_precision_flag_on_other_types(bp):
    cell = "16_1/2_z24"
    ref = fc.reference(cell, "sumprod2")
    ch = np.ascontiguousarray(ref.CH)
    lib = bp.load_bp_library()
    # a context without layers: the binary32 layered types are argument errors, as the binary64 ones are
    c = fc.make_code(cell)
    for algo in (bp.LB_LAYERED_SUMPROD2 | LB_F32, bp.LB_LAYERED_MINSUM | LB_F32):
        for max_iter in (0, 5):
            rc, msg, _, _ = _raw_decode(lib, c, ch, algo, max_iter)
            assert rc == -1 and "layers" in msg, (rc, msg)
        assert lib.lb_stage(c._context(), len(ch), ch.ctypes.data_as(_DP)) == 0
        assert lib.lb_run(c._context(), len(ch), algo, 0.7, 5) == -1
    # the flag on a flooding type is unsupported, whatever max_iter, with or without layers
    before = [c.decode_batch(ch, a, max_iter=12) for a in ("sumprod2", "minsum", "sumprod")]
    for layers_set in (False, True):
        if layers_set:
            c.set_layers(np.arange(0, c.Nc + 1, c.z))
        for algo in (bp.LB_SUMPROD2, bp.LB_SUMPROD, bp.LB_MINSUM):
            for max_iter in (0, 5):
                rc, msg, app, it = _raw_decode(lib, c, ch, algo | LB_F32, max_iter)
                assert rc == -5 and "binary32" in msg and "layered" in msg, (rc, msg)
                assert (app == 7.0).all() and (it == -3).all()  # nothing written
            assert lib.lb_run(c._context(), len(ch), algo | LB_F32, 0.7, 5) == -5
            with pytest.raises(bp.LdpcBpError) as e:
                bp._check(lib.lb_run(c._context(), len(ch), algo | LB_F32, 0.7, 5))
            assert e.value.code == -5
    # numbers outside the five types stay argument errors, with the flag and without
    for algo in (5, 6, 5 | LB_F32, 7 | LB_F32, LB_F32 << 1, (LB_F32 << 1) | 3, -1, -LB_F32):
        rc, msg, _, _ = _raw_decode(lib, c, ch, algo, 5)
        assert rc == -1, (algo, rc, msg)
    # and the context decodes as before
    after = [c.decode_batch(ch, a, max_iter=12) for a in ("sumprod2", "minsum", "sumprod")]
    for (a0, i0), (a1, i1) in zip(before, after):
        assert np.array_equal(a0, a1, equal_nan=True) and np.array_equal(i0, i1)
    # the names: decode keeps the reference's three
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        c.decode(ch[0], "layered_sumprod2_f32")
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        c.decode_batch(ch, "sumprod2_f32")
    with pytest.raises(KeyError):
        c.run_buffers(len(ch), "minsum_f32")


@pytest.mark.parametrize("lds", [None, 0])
@pytest.mark.parametrize("cell", ["16_1/2_z24", "16_5/6_z300"])
def test_binary64_decodes_are_untouched_by_binary32_ones(bp, monkeypatch, cell, lds):
    """The same binary64 layered and flooding decodes before and after binary32 ones on one context, host- and
    device-sized: identical bits.  The message slices in HBM are shared: the flooding tail's two slots, the
    binary64 layered r (5/6 z=300, or everything with LDPC_BP_LAYERED_LDS=0), the binary32 r and app as floats."""
    if lds is not None:
        monkeypatch.setenv("LDPC_BP_LAYERED_LDS", str(lds))
    ref = fc.reference(cell, "sumprod2")
    c = fc.make_code(cell)
    types = ("sumprod2", "minsum", "layered_sumprod2", "layered_minsum")

    def run_all():
        return [c.decode_batch(ref.CH, a, max_iter=12) for a in types] + \
            [_staged(bp, c, ref.CH, a, 12) for a in ("sumprod2", "layered_sumprod2")]

    before = run_all()
    info0, linfo0 = c.info(), c.layer_info()
    for a in fc.ALGOS:
        c.decode_batch(ref.CH, _dectype(a), max_iter=12)
        _staged(bp, c, ref.CH[::-1], _dectype(a), 3)
    assert c.info() == info0 and c.layer_info() == linfo0
    for (a0, i0), (a1, i1) in zip(before, run_all()):
        assert np.array_equal(a0, a1) and np.array_equal(np.signbit(a0), np.signbit(a1)) and np.array_equal(i0, i1)
    # and the binary32 ones after the binary64 ones are what they were
    app, it = c.decode_batch(ref.CH, "layered_minsum_f32", max_iter=12)
    got = [fc.trace(ref.c, ch, "minsum", ref.layers) for ch in ref.CH]  # the minsum statement on these words
    assert np.array_equal(it, [g[0] for g in got])
    assert np.array_equal(app, np.array([g[1][-1] for g in got]))


def test_mc_blocks_f32_equal_decode_batch(bp):
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
    for dectype in ("layered_sumprod2_f32", "layered_minsum_f32"):
        be0, it0 = want(u, w, dectype)
        assert it0.min() >= 1 and len(set(it0.tolist())) > 2
        be, it = c.mc_blocks(u, w, sigma, dectype=dectype, batch=5)
        assert np.array_equal(be, be0) and np.array_equal(it, it0)
        be0, it0 = want(ud, wd, dectype)
        be, it = c.mc_blocks_seeds(seeds, sigma, dectype=dectype, batch=5)
        assert np.array_equal(be, be0) and np.array_equal(it, it0)
        be, it = ldpc_mc.mc_ldpc(c, sigma, seeds, batch=7, dectype=dectype, draws="device")
        assert np.array_equal(be, be0) and np.array_equal(it, it0)


def test_sim_ldpc_mc_f32(bp):
    import sparc_ldpc_amd as sp
    lp = sp.LDPCParams("802.16", "1/2", 24)
    never = 10 ** 9
    kw = dict(MIN_ERRORS=never, MAX_BLOCKS=64, batch=32)
    flood = sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, **kw)
    c = bp.code("802.16", "1/2", 24)
    for draws in ("host", "device"):
        lay = sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, dectype="layered_sumprod2_f32", draws=draws, **kw)
        assert lay["blocks"] == flood["blocks"] == 64  # the same blocks consumed as the default
        # its counts: those of decode_batch on the same blocks' LLRs
        from sparc_ldpc_amd import ldpc_mc
        u, w = (ldpc_mc._draw_blocks if draws == "host" else
                lambda s, K, N, ch: ldpc_mc.draw_blocks_device(c, s))(np.arange(64), c.K, c.N, "awgn")
        x = c.encode_batch(u)
        app, it = c.decode_batch((2.0 / llc.SIM_SIGMA ** 2) * ((1.0 - 2.0 * x) + llc.SIM_SIGMA * w),
                                 "layered_sumprod2_f32")
        be = ((app < 0.0) != x).sum(axis=1)
        assert lay["bit_errors"] == int(be.sum()) and lay["block_errors"] == int((be > 0).sum())
        assert lay["nit_total"] == int(it.sum()) and 0 < lay["nit_total"] < flood["nit_total"]
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        sp.sim_ldpc_mc(lp, llc.SIM_SIGMA, dectype="layered_f32", **kw)


def test_awgn_and_bsc_sweeps_take_the_binary32_names(bp):
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc
    kw = dict(N_MEASUREMENTS=2, C_AWGN_OFFSET=6.0, MIN_ERRORS=3, MAX_BLOCKS=24, batch=8)
    flood = ldpc_awgn.sim("802.16", "1/2", 24, **kw)
    lay = ldpc_awgn.sim("802.16", "1/2", 24, dectype="layered_sumprod2_f32", **kw)
    assert len(lay) == len(flood) == 2 and lay[0][:4] == flood[0][:4]
    assert lay[0][8] / lay[0][4] < flood[0][8] / flood[0][4]  # nit_total per block: sweeps against iterations
    res, parray = ldpc_bsc.sim("802.16", "1/2", 24, repeats=6, dectype="layered_minsum_f32")
    assert len(res) == len(parray) == 10 and res[-1] == 0.0  # p = 0.001: no bit error left
