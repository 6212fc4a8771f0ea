"""GPU: the fixed-point layered min-sum kernels k_bplq / k_bplsq (LB_FIXED, the
``quant`` keyword) against their NumPy statement
(tests/ldpc_fixed_ref.py).  Integer arithmetic has one right answer: every
comparison is array_equal on app (there is only +0) and exact sweep counts,
against the statement's traced run; the Monte-Carlo layers are compared with
decode_batch(quant=...) on the same LLRs and with each other, block by block.
The words are the layered tests' own plus the binary32 tests' clamp word; what
they must satisfy is asserted here from the statement alone, before any device
call."""
import ctypes as ct

import numpy as np
import pytest

import ldpc_fixed_cases as qc
import ldpc_fixed_ref as qr

pytestmark = pytest.mark.gpu

_IP = ct.POINTER(ct.c_int)
_DP = ct.POINTER(ct.c_double)
_LP = ct.POINTER(ct.c_long)
LB_F32, LB_FIXED = 0x100, 0x400
FIXED = 4 | LB_FIXED  # LB_LAYERED_MINSUM | LB_FIXED
DT = "layered_minsum"


@pytest.fixture(scope="module")
def bp():
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible: -m gpu tests need an MI355X"
    assert ldpc.LB_FIXED == LB_FIXED and ldpc.LB_LAYERED_MINSUM == 4
    return ldpc


def _equal(app, it, rapp, rit, what):
    assert np.array_equal(it, rit), (what, it, rit)
    assert np.array_equal(app, rapp), (what, np.argwhere(app != rapp)[:4])
    assert np.array_equal(np.signbit(app), np.signbit(rapp)), what


def _staged(bp, c, ch, k, corr, quant):
    B = ch.shape[0]
    c.device_buffers(B)
    assert bp.load_bp_library().lb_stage(c._context(), B, np.ascontiguousarray(ch).ctypes.data_as(_DP)) == 0
    c.run_buffers(B, DT, corr, k, quant=quant)
    return c.fetch_buffers(B)


def _check_info(c, cell, widths, threads=None, lanes=None):
    info = c.fixed_info()
    want_threads, want_lanes = qc.CELLS[cell]
    assert (info["frac_bits"], info["msg_bits"], info["app_bits"]) == tuple(widths), info
    assert info["threads"] == (threads or want_threads) and info["lanes"] == (lanes or want_lanes), info
    assert info["lds_bytes"] == qc.lds_bytes(c) and info["fits"] == 1 and info["resident"] >= 1, info
    # what a CU can hold at most: 160 KB of LDS, 2048 threads
    assert info["resident"] <= min(160 * 1024 // info["lds_bytes"], 2048 // info["threads"]), info
    return info


@pytest.mark.parametrize("cell", qc.SMALL)
def test_truncated_decodes_against_statement(bp, cell):
    qc.check_preconditions(cell)
    c = qc.make_code(cell)
    assert c.fixed_info() == dict(frac_bits=2, msg_bits=6, app_bits=8, threads=0, lanes=0, lds_bytes=0, resident=0,
                                  fits=0)  # nothing planned before the layers are set
    call = 0
    for widths in qc.WIDTHS:
        for corr in qc.CORRS:
            ref = qc.reference(cell, widths, corr)
            W = len(ref.CH)
            for k in qc.KS:
                # host pointers and staged buffers in turn; another order and another number of words every call
                idx = np.roll(np.arange(W), call)[:W - call % 3]
                if call % 2 == 0:
                    app, it = c.decode_batch(ref.CH[idx], DT, corr, k, quant=widths)
                else:
                    app, it = _staged(bp, c, ref.CH[idx], k, corr, widths)
                call += 1
                _equal(app, it, *ref.at(k, idx), (widths, corr, k, idx.tolist()))
        info = _check_info(c, cell, widths)
    print(f"\nfixed {cell}: sweeps at (2, 6, 8) {qc.reference(cell).its.tolist()} "
          f"clips at (1, 4, 6) {qc.reference(cell, (1, 4, 6)).clips} {info}")


def test_no_clip_fires_on_the_pin_words_and_the_decoder_is_binary64_minsum_there(bp):
    """(3, 8, 16) and (2, 8, 16) at corr_factor 1 on the pin words: the fixed-point kernel, its statement and the
    binary64 layered min-sum kernel give the same app and sweeps."""
    for cell in ("16_1/2_z24", "16_5/6_z192"):
        c = qc.make_code(cell)
        CH = qc.pin_words(cell, c)
        g = qc.layers(cell)
        want = []
        for widths in ((3, 8, 16), qc.PIN_WIDTHS):
            clips = {}
            want = [qr.decode(ch, None, None, None, None, *widths, corr_factor=1.0, max_it=qc.PIN_SWEEPS, layers=g,
                              clips=clips) for ch in CH]
            assert sum(clips.values()) == 0, (cell, widths, clips)
            app, it = c.decode_batch(CH, DT, 1.0, qc.PIN_SWEEPS, quant=widths)
            _equal(app, it, np.array([w[0] for w in want]), np.array([w[1] for w in want]), (cell, widths))
        app64, it64 = c.decode_batch(CH, DT, 1.0, qc.PIN_SWEEPS)
        _equal(app64, it64, np.array([w[0] for w in want]), np.array([w[1] for w in want]), (cell, "binary64"))


def test_more_words_than_the_chip_holds(bp):
    """802.16 5/6 z=192: the two AWGN words alone, then 600 words (every word of the cell 120 times, shuffled):
    more workgroups than are resident at once."""
    cell = "16_5/6_z192"
    qc.check_preconditions(cell)
    c = qc.make_code(cell)
    labels = qc.reference(cell).labels
    two = np.array([i for i, lab in enumerate(labels) if lab == "awgn"])
    assert len(two) == 2 and len(labels) == 5  # AWGN x 2, noiseless, hopeless, clamp
    idx = np.random.RandomState(7).permutation(np.repeat(np.arange(5), 120))
    for widths in qc.WIDTHS:
        ref = qc.reference(cell, widths)
        for k in (3, 12):
            _equal(*c.decode_batch(ref.CH[two], DT, 0.75, k, quant=widths), *ref.at(k, two), (widths, k, "two"))
            _equal(*c.decode_batch(ref.CH[idx], DT, 0.75, k, quant=widths), *ref.at(k, idx), (widths, k, "600 host"))
        _equal(*_staged(bp, c, ref.CH[idx], 12, 0.75, widths), *ref.at(12, idx), (widths, "600 staged"))
    info = _check_info(c, cell, qc.WIDTHS[-1])
    assert info["lds_bytes"] == 2 * 4608 + 15360 == 24576
    print(f"\nfixed {cell}: {info}")


def test_the_110_kb_image(bp):
    """802.16 5/6 z=864: app and r of a word are 110 592 bytes of LDS, one workgroup a CU, 864 checks a layer
    strided over 1024 threads; binary64 keeps both in HBM here."""
    cell = "16_5/6_z864"
    qc.check_preconditions(cell)
    c = qc.make_code(cell)
    two = np.array([i for i, lab in enumerate(qc.reference(cell).labels) if lab == "awgn"])
    for widths in qc.WIDTHS:
        ref = qc.reference(cell, widths)
        _equal(*c.decode_batch(ref.CH[two], DT, 0.75, 12, quant=widths), *ref.at(12, two), (widths, "two"))
        _equal(*_staged(bp, c, ref.CH[::-1], 6, 0.75, widths), *ref.at(6, range(len(ref.CH))[::-1]), (widths, "all"))
    info = _check_info(c, cell, qc.WIDTHS[-1])
    assert info["lds_bytes"] == 110592 and info["resident"] == 1 and c.layer_info()["lds_messages"] == 0
    print(f"\nfixed {cell}: {info}")


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("cell", ["syn_dc8", "16_1/2_z24", "16_5/6_z24", "syn_dc32"])
def test_lanes_per_check(bp, monkeypatch, cell, lanes):
    """LDPC_BP_FIXED_LANES: every group width on every check-degree class (syn_dc8's checks of degree 2 and 3
    have fewer edges than a group has lanes); the same bits."""
    monkeypatch.setenv("LDPC_BP_FIXED_LANES", str(lanes))
    c = qc.make_code(cell)
    for widths in ((2, 6, 8), (1, 4, 6)):
        ref = qc.reference(cell, widths)
        for k in (3, 12):
            _equal(*c.decode_batch(ref.CH, DT, 0.75, k, quant=widths), *ref.at(k), (lanes, widths, k))
        _check_info(c, cell, widths, threads=min(1024, -(-c.z * lanes // 64) * 64), lanes=lanes)


@pytest.mark.parametrize("threads", [64, 128])
def test_thread_counts(bp, monkeypatch, threads):
    """LDPC_BP_FIXED_THREADS at 802.16 1/2 z=96: a layer's 96 checks (4 lanes each) strided over 64 and 128
    threads, and with 16 lanes a check over 4 and 8 groups."""
    cell = "16_1/2_z96"
    monkeypatch.setenv("LDPC_BP_FIXED_THREADS", str(threads))
    for lanes in (None, 16):
        if lanes:
            monkeypatch.setenv("LDPC_BP_FIXED_LANES", str(lanes))
        c = qc.make_code(cell)
        for widths in ((2, 6, 8), (1, 4, 6)):
            ref = qc.reference(cell, widths)
            _equal(*c.decode_batch(ref.CH, DT, 0.75, 12, quant=widths), *ref.at(12), (threads, lanes, widths))
            _check_info(c, cell, widths, threads=threads, lanes=lanes)


def _raw_decode(lib, ctx, ch, algo, max_iter, corr=0.75):
    app = np.full_like(ch, 7.0)
    it = np.full(len(ch), -3, dtype=np.intc)
    rc = lib.lb_decode(ctx, len(ch), ch.ctypes.data_as(_DP), app.ctypes.data_as(_DP), it.ctypes.data_as(_IP), algo,
                       corr, max_iter)
    return rc, lib.lb_last_error().decode(), app, it


def test_set_fixed_between_decodes(bp):
    cell = "16_1/2_z24"
    lib = bp.load_bp_library()
    c = qc.make_code(cell)
    ch = np.ascontiguousarray(qc.reference(cell).CH)
    c.set_layers(np.arange(0, c.Nc + 1, c.z))
    # never called: (2, 6, 8)
    rc, _, app, it = _raw_decode(lib, c._context(), ch, FIXED, 12)
    assert rc == 0
    _equal(app, it, *qc.reference(cell, (2, 6, 8)).at(12), "default widths")
    for widths in ((1, 4, 6), (3, 8, 16), (0, 2, 2), (8, 8, 16)):
        c.set_fixed(*widths)
        info = _check_info(c, cell, widths)
        rc, _, app, it = _raw_decode(lib, c._context(), ch, FIXED, 12)
        assert rc == 0
        if widths in qc.WIDTHS:
            want = qc.reference(cell, widths).at(12)
        else:
            runs = [qr.decode(x, None, None, None, None, *widths, max_it=12, layers=qc.layers(cell)) for x in ch]
            want = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
        _equal(app, it, *want, widths)
        # out of range: -1, the widths and the plan stay, and the next decode is the same
        for bad in ((-1, 6, 8), (9, 6, 8), (2, 1, 8), (2, 9, 9), (2, 6, 5), (2, 6, 17)):
            assert lib.lb_set_fixed(c._context(), *bad) == -1 and b"widths" in lib.lb_last_error()
            with pytest.raises(AssertionError):
                c.set_fixed(*bad)
        assert c.fixed_info() == info
        rc, _, app2, it2 = _raw_decode(lib, c._context(), ch, FIXED, 12)
        assert rc == 0 and np.array_equal(app2, app) and np.array_equal(it2, it)
    # quant=True is the default widths, whatever was set before
    _equal(*c.decode_batch(ch, DT, 0.75, 12, quant=True), *qc.reference(cell).at(12), "quant=True")
    # max_iter = 0: the channel itself, unquantised, sign of zero and all
    for app, it in (c.decode_batch(ch, DT, 0.75, 0, quant=(0, 2, 2)), _staged(bp, c, ch, 0, 0.75, (0, 2, 2))):
        assert np.array_equal(app, ch) and np.array_equal(np.signbit(app), np.signbit(ch)) and not it.any()


def test_rejections_write_nothing(bp):
    cell = "16_1/2_z24"
    lib = bp.load_bp_library()
    ch = np.ascontiguousarray(qc.reference(cell).CH)
    B = len(ch)

    def refused(c, algo, max_iter, corr, code, *words):
        rc, msg, app, it = _raw_decode(lib, c._context(), ch, algo, max_iter, corr)
        assert rc == code and all(w in msg for w in words), (algo, max_iter, corr, rc, msg)
        assert (app == 7.0).all() and (it == -3).all()  # nothing written
        assert lib.lb_stage(c._context(), B, ch.ctypes.data_as(_DP)) == 0
        assert lib.lb_run(c._context(), B, algo, corr, max_iter) == code
        d_ch, d_app, d_it = c.device_buffers(B)
        assert lib.lb_decode_device(c._context(), B, d_ch, d_app, d_it, algo, corr, max_iter) == code

    # no layers set: an argument error, as for the other layered types
    c = qc.make_code(cell)
    for max_iter in (0, 5):
        refused(c, FIXED, max_iter, 0.75, -1, "layers")
    before = [c.decode_batch(ch, a, max_iter=12) for a in ("sumprod2", "minsum")]
    for layers_set in (False, True):
        if layers_set:
            c.set_layers(np.arange(0, c.Nc + 1, c.z))
        for max_iter in (0, 5):
            # on layered sumprod2 and on the flooding types: unsupported
            for algo in (bp.LB_LAYERED_SUMPROD2, bp.LB_SUMPROD2, bp.LB_SUMPROD, bp.LB_MINSUM):
                refused(c, algo | LB_FIXED, max_iter, 0.75, -5, "fixed-point", "layered min-sum")
            # with binary32: an argument error, on any type
            for algo in (bp.LB_LAYERED_MINSUM, bp.LB_LAYERED_SUMPROD2, bp.LB_MINSUM):
                refused(c, algo | LB_FIXED | LB_F32, max_iter, 0.75, -1)
            # 0x200 and numbers outside the five types stay argument errors
            for algo in (4 | 0x200, 4 | 0x200 | LB_FIXED, 5 | LB_FIXED, LB_FIXED, LB_FIXED << 1, -LB_FIXED):
                refused(c, algo, max_iter, 0.75, -1 if algo != LB_FIXED else -5)
    # rint(16 corr_factor) outside 1..16, or NaN (also at max_iter = 0)
    for corr in (0.0, 1 / 32, -0.75, 1.04, 2.0, float("nan"), float("inf")):
        for max_iter in (0, 5):
            refused(c, FIXED, max_iter, corr, -1, "corr_factor")
    with pytest.raises(AssertionError):
        c.decode_batch(ch, DT, 0.0, quant=True)
    for corr in (1.03, 1 / 16, 0.04):  # alpha 16, 1, 1 (0.64 rounds to 1)
        rc, _, app, it = _raw_decode(lib, c._context(), ch, FIXED, 3, corr)
        runs = [qr.decode(x, None, None, None, None, corr_factor=corr, max_it=3, layers=qc.layers(cell)) for x in ch]
        assert rc == 0
        _equal(app, it, np.array([r[0] for r in runs]), np.array([r[1] for r in runs]), corr)
    # the Monte-Carlo entries refuse the same way and return nothing
    from sparc_ldpc_amd import ldpc_mc
    seeds = np.arange(5)
    for call in (lambda **kw: c.mc_blocks_seeds(seeds, 0.8, dectype=DT, **kw),
                 lambda **kw: c.mc_stream_seeds(seeds, 0.8, dectype=DT, **kw),
                 lambda **kw: c.mc_blocks(*ldpc_mc._draw_blocks(seeds, c.K, c.N), 0.8, dectype=DT, **kw)):
        with pytest.raises(AssertionError, match="corr_factor"):
            call(corr_factor=1.04, quant=True)
        with pytest.raises(AssertionError, match="widths"):
            call(quant=(2, 9, 9))
    errs, its, out = np.full(5, -3, np.intc), np.full(5, -3, np.intc), (ct.c_int64 * 4)()
    s32 = np.ascontiguousarray(seeds, dtype=np.uint32)
    for algo, code in ((bp.LB_LAYERED_SUMPROD2 | LB_FIXED, -5), (FIXED | LB_F32, -1), (bp.LB_MINSUM | LB_FIXED, -5)):
        c._set_encoder()
        rc = lib.lb_mc_stream_seeds(c._context(), 5, s32.ctypes.data_as(ct.POINTER(ct.c_uint32)), c.K, 0.8, 0, 4, 0, 0,
                                    algo, 0.75, 5, errs.ctypes.data_as(_IP), its.ctypes.data_as(_IP), out)
        assert rc == code and (errs == -3).all() and (its == -3).all(), (algo, rc)
        rc = lib.lb_mc_run_seeds(c._context(), 5, s32.ctypes.data_as(ct.POINTER(ct.c_uint32)), c.K, 0.8, 0, 4, algo,
                                 0.75, 5, errs.ctypes.data_as(_IP), its.ctypes.data_as(_IP))
        assert rc == code and (errs == -3).all() and (its == -3).all(), (algo, rc)
    # and the context decodes as before
    after = [c.decode_batch(ch, a, max_iter=12) for a in ("sumprod2", "minsum")]
    for (a0, i0), (a1, i1) in zip(before, after):
        assert np.array_equal(a0, a1) and np.array_equal(i0, i1)
    _equal(*c.decode_batch(ch, DT, 0.75, 12, quant=True), *qc.reference(cell).at(12), "after the refusals")
    # the names: decode keeps the reference's signature
    with pytest.raises(TypeError):
        c.decode(ch[0], "minsum", 0.7, quant=True)


def test_an_image_that_does_not_fit_is_unsupported(bp):
    """A synthetic graph of 50 000 variables of degree 2 and 25 000 checks of degree 4 in two layers:
    2 Nv + Nmsg = 200 000 bytes, more than a workgroup's LDS.  There is no HBM layout."""
    lib = bp.load_bp_library()
    Nv, Nc = 50000, 25000
    vdeg = np.full(Nv, 2, dtype=np.int64)
    cdeg = np.full(Nc, 4, dtype=np.int64)
    intrlv = np.empty(2 * Nv, dtype=np.int64)
    intrlv[0::2] = np.arange(Nv)  # port 0 of variable j: message j, in check j // 4 (layer 0)
    intrlv[1::2] = Nv + (np.arange(Nv) * 7919) % Nv  # port 1: a message of layer 1, variables spread over its checks
    ctx = ct.c_void_p()
    assert lib.lb_create(ct.byref(ctx), vdeg.ctypes.data_as(_LP), cdeg.ctypes.data_as(_LP), intrlv.ctypes.data_as(_LP),
                         Nv, Nc, 2 * Nv, 0) == 0
    try:
        fc = np.array([0, Nc // 2, Nc], dtype=np.intc)
        assert lib.lb_set_layers(ctx, 2, fc.ctypes.data_as(_IP)) == 0
        out = (ct.c_int64 * 8)()
        assert lib.lb_fixed_info(ctx, out) == 0
        assert list(out) == [2, 6, 8, 1024, 1, 200000, 0, 0], list(out)
        ch = np.ones((1, Nv))
        for max_iter in (0, 5):
            rc, msg, app, it = _raw_decode(lib, ctx, ch, FIXED, max_iter)
            assert rc == -5 and "fit" in msg and (app == 7.0).all() and (it == -3).all(), (rc, msg)
        # the binary64 layered decoder takes the graph (messages in HBM): an all-positive word is a codeword
        rc, _, app, it = _raw_decode(lib, ctx, ch, 4, 5)
        assert rc == 0 and np.array_equal(app, ch) and it[0] == 0
    finally:
        lib.lb_destroy(ctx)


@pytest.mark.parametrize("cell", ["16_1/2_z24", "16_5/6_z300"])
def test_other_decoders_are_untouched_by_fixed_point_ones(bp, cell):
    """Binary64 and binary32 layered and flooding decodes on one context, host- and device-sized, before and
    after fixed-point ones: identical bits."""
    c = qc.make_code(cell)
    import ldpc_layered_cases as llc
    CH = qc.words(cell, c)[1] if cell in qc.CELLS else llc.words(cell, "minsum", c)[1]  # (5/6 z=300: two AWGN words)
    types = ("sumprod2", "minsum", "layered_sumprod2", "layered_minsum", "layered_sumprod2_f32", "layered_minsum_f32")

    def staged(a, k):
        c.device_buffers(len(CH))
        assert bp.load_bp_library().lb_stage(c._context(), len(CH), np.ascontiguousarray(CH).ctypes.data_as(_DP)) == 0
        c.run_buffers(len(CH), a, max_iter=k)
        return c.fetch_buffers(len(CH))

    def run_all():
        return [c.decode_batch(CH, a, max_iter=12) for a in types] + \
            [staged(a, 12) for a in ("sumprod2", "layered_sumprod2", "layered_minsum_f32")]

    before = run_all()
    info0, linfo0, finfo0 = c.info(), c.layer_info(), c.layer_info("f32")
    g = qr.Layers(c.vdeg, c.cdeg, c.intrlv, qr.code_layers(c))
    for widths in ((2, 6, 8), (1, 4, 6)):
        runs = [qr.decode(x, None, None, None, None, *widths, max_it=12, layers=g) for x in CH]
        want = np.array([r[0] for r in runs]), np.array([r[1] for r in runs])
        _equal(*c.decode_batch(CH, DT, 0.75, 12, quant=widths), *want, widths)
        _equal(*_staged(bp, c, CH, 12, 0.75, widths), *want, widths)
    assert c.info() == info0 and c.layer_info() == linfo0 and c.layer_info("f32") == finfo0
    for (a0, i0), (a1, i1) in zip(before, run_all()):
        assert np.array_equal(a0, a1, equal_nan=True) and np.array_equal(np.signbit(a0), np.signbit(a1))
        assert np.array_equal(i0, i1)


# ---- Monte-Carlo ----------------------------------------------------------------
SEEDS = np.arange(100, 400)  # 300 blocks
MC = {  # name -> (standard, rate, z, channel, noise levels to try)
    "16-5/6-z24": ("802.16", "5/6", 24, "awgn", (0.50, 0.52, 0.54, 0.56, 0.58, 0.60, 0.62)),
    "11n-1/2-z27": ("802.11n", "1/2", 27, "awgn", (0.80, 0.84, 0.88, 0.92, 0.96, 1.00)),
    "bsc": ("802.11n", "1/2", 27, "bsc", (0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.10, 0.11)),
}
MC_WIDTHS = ((2, 6, 8), (1, 4, 6))
_mc = {}


def _mc_case(bp, name):
    """(code, channel, a, per widths the batch path's (errs, iters)): the first noise level of the case's fixed
    ladder at which the batch path leaves at least 20 clean and 20 failed blocks at every widths."""
    if name not in _mc:
        std, rate, z, channel, ladder = MC[name]
        c = bp.code(std, rate, z)
        for a in ladder:
            got = {w: c.mc_blocks_seeds(SEEDS, a, channel, 64, DT, 0.75, quant=w) for w in MC_WIDTHS}
            if all(min(int((be > 0).sum()), int((be == 0).sum())) >= 20 for be, _ in got.values()):
                for be, it in got.values():
                    be.setflags(write=False)
                    it.setflags(write=False)
                _mc[name] = (c, channel, a, got)
                break
        assert name in _mc, "no noise level of the ladder leaves both clean and failed blocks"
    return _mc[name]


@pytest.mark.parametrize("name", sorted(MC))
def test_mc_blocks_equal_decode_batch(bp, name):
    from sparc_ldpc_amd import ldpc_mc
    c, channel, a, batch = _mc_case(bp, name)
    K = ldpc_mc.info_bits(c, channel)

    def llrs(u, w):
        x = c.encode_batch(u) if K else np.zeros((len(w), c.N), dtype=np.int64)
        if channel == "awgn":
            return x, (2.0 / a ** 2) * ((1.0 - 2.0 * x) + a * w)
        return x, np.where(w < a, -1.0, 1.0) * np.log((1.0 - a) / a)

    u, w = ldpc_mc._draw_blocks(SEEDS, K, c.N, channel)
    ud, wd = ldpc_mc.draw_blocks_device(c, SEEDS, channel)
    for widths in MC_WIDTHS:
        x, ch = llrs(u, w)
        app, it0 = c.decode_batch(ch, DT, 0.75, quant=widths)
        be0 = ((app < 0.0) != x).sum(axis=1)
        be, it = c.mc_blocks(u, w, a, channel, 77, DT, 0.75, quant=widths)
        assert np.array_equal(be, be0) and np.array_equal(it, it0), widths
        x, ch = llrs(ud, wd)
        app, it0 = c.decode_batch(ch, DT, 0.75, quant=widths)
        be0 = ((app < 0.0) != x).sum(axis=1)
        assert np.array_equal(batch[widths][0], be0) and np.array_equal(batch[widths][1], it0), widths
        be, it = ldpc_mc.mc_ldpc(c, a, SEEDS, channel, 50, DT, draws="device", quant=widths)  # (corr_factor 0.7)
        app, it0 = c.decode_batch(ch, DT, 0.7, quant=widths)
        assert np.array_equal(be, ((app < 0.0) != x).sum(axis=1)) and np.array_equal(it, it0), widths
        print(f"{name} a={a} {widths}: failed={int((be0 > 0).sum())} mean sweeps={it0.mean():.2f}")


@pytest.mark.parametrize("name", sorted(MC))
def test_stream_equals_batch_per_block(bp, name):
    c, channel, a, batch = _mc_case(bp, name)
    for widths in MC_WIDTHS:
        be0, it0 = batch[widths]
        for chunk, slots in [(64, 3), (37, 1), (300, 0)]:
            be, it, info = c.mc_stream_seeds(SEEDS, a, channel, chunk, DT, 0.75, slots=slots, quant=widths)
            np.testing.assert_array_equal(be, be0, err_msg=f"{widths} chunk {chunk} slots {slots}")
            np.testing.assert_array_equal(it, it0, err_msg=f"{widths} chunk {chunk} slots {slots}")
            assert info["used"] == info["decoded"] == 300 and info["chunks"] == -(-300 // chunk), info
            assert 1 <= info["slots"] <= min(chunk, 300) and (slots == 0 or info["slots"] == min(slots, chunk)), info
        for max_iter in (0, 3):
            be0, it0 = c.mc_blocks_seeds(SEEDS, a, channel, 64, DT, 0.75, max_iter, quant=widths)
            assert it0.max() == max_iter and (be0 > 0).any()
            for chunk, slots in [(64, 3), (37, 1), (300, 0)]:
                be, it, _ = c.mc_stream_seeds(SEEDS, a, channel, chunk, DT, 0.75, max_iter, slots=slots, quant=widths)
                np.testing.assert_array_equal(be, be0, err_msg=f"{widths} max_iter {max_iter} chunk {chunk}")
                np.testing.assert_array_equal(it, it0, err_msg=f"{widths} max_iter {max_iter} chunk {chunk}")


@pytest.mark.parametrize("std,rate,z,sigma,degrees", [("802.16", "3/4", 24, 0.62, [14, 15]),
                                                      ("802.11n", "5/6", 27, 0.54, [22])])
def test_stream_equals_batch_in_degree_classes_16_and_32(bp, std, rate, z, sigma, degrees):
    """The batch / stream pairs of the two check-degree classes that no case of MC reaches: 16 (802.16 3/4,
    checks of 14 and 15 edges) and 32 (802.11n 5/6, 22 edges)."""
    c = bp.code(std, rate, z)
    assert sorted(set(np.asarray(c.cdeg).tolist())) == degrees
    be0, it0 = c.mc_blocks_seeds(SEEDS, sigma, "awgn", 64, DT, 0.75, quant=True)
    failed, clean = int((be0 > 0).sum()), int((be0 == 0).sum())
    print(f"{std} {rate} z={z} sigma={sigma} fixed point: failed={failed} clean={clean} mean sweeps={it0.mean():.2f}")
    assert failed and clean, "the case must hold both clean and failed blocks"
    for chunk, slots in [(64, 3), (300, 0)]:
        be, it, info = c.mc_stream_seeds(SEEDS, sigma, "awgn", chunk, DT, 0.75, slots=slots, quant=True)
        np.testing.assert_array_equal(be, be0, err_msg=f"chunk {chunk} slots {slots}")
        np.testing.assert_array_equal(it, it0, err_msg=f"chunk {chunk} slots {slots}")
        assert info["used"] == info["decoded"] == 300 and info["chunks"] == -(-300 // chunk), info


def test_stream_stop_rule_and_python_layers(bp):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_awgn, ldpc_bsc
    c, channel, a, batch = _mc_case(bp, "16-5/6-z24")
    be0, it0 = batch[(2, 6, 8)]
    cum = np.cumsum(be0 > 0)
    min_errors = 5
    nstar = int(np.argmax(cum >= min_errors)) + 1
    assert cum[-1] >= 20 and nstar < 300
    for chunk, slots in ((16, 2), (64, 0)):
        be, it, info = c.mc_stream_seeds(SEEDS, a, channel, chunk, DT, 0.75, min_errors=min_errors, slots=slots,
                                         quant=True)
        assert info["used"] == nstar, info
        np.testing.assert_array_equal(be[:nstar], be0[:nstar])
        np.testing.assert_array_equal(it[:nstar], it0[:nstar])
        skipped = it[nstar:] == -1
        assert np.all(be[nstar:][skipped] == 0) and info["decoded"] == int((it != -1).sum())
        np.testing.assert_array_equal(be[nstar:][~skipped], be0[nstar:][~skipped])
        np.testing.assert_array_equal(it[nstar:][~skipped], it0[nstar:][~skipped])
    lp = sp.LDPCParams("802.16", "5/6", 24)
    for rule in ((5, 400), (1000, 137)):
        kw = dict(MIN_ERRORS=rule[0], MAX_BLOCKS=rule[1], seed0=9, batch=50, draws="device", dectype=DT, quant=(1, 4, 6))
        want = sp.sim_ldpc_mc(lp, a, **kw)
        got = sp.sim_ldpc_mc(lp, a, stream=True, **kw)
        assert got == want and repr(got["ber"]) == repr(want["ber"]) and want["blocks"] <= rule[1]
    kw = dict(N_MEASUREMENTS=2, MIN_ERRORS=3, MAX_BLOCKS=40, seed0=3, batch=16, draws="device", dectype=DT, quant=True)
    assert ldpc_awgn.sim("802.16", "5/6", 24, stream=True, **kw) == ldpc_awgn.sim("802.16", "5/6", 24, **kw)
    kw = dict(repeats=20, seed0=1, draws="device", dectype=DT, quant=True)
    res0, p0 = ldpc_bsc.sim("802.16", "5/6", 24, **kw)
    res1, p1 = ldpc_bsc.sim("802.16", "5/6", 24, stream=True, **kw)
    assert res0 == res1 and np.array_equal(p0, p1) and res0[-1] == 0.0


def test_sim_ldpc_mc_against_the_statement(bp):
    """802.16 1/2 z=24, blocks 0..63 at SIM_SIGMA: the dict is a sequential consumption of the statement's
    per-block results (sim_ldpc_mc decodes at corr_factor 0.7, up to 200 sweeps)."""
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc_mc
    from sparc_ldpc_amd.harness import consume_in_seed_order
    lp = sp.LDPCParams("802.16", "1/2", 24)
    c = qc.make_code("16_1/2_z24")
    g = qc.layers("16_1/2_z24")
    sigma = qc.SIM_SIGMA
    u, w = ldpc_mc._draw_blocks(np.arange(64), c.K, c.N, "awgn")
    x = c.encode_batch(u)
    CH = (2.0 / sigma ** 2) * ((1.0 - 2.0 * x) + sigma * w)
    for widths in ((2, 6, 8), (1, 4, 6)):
        runs = [qr.decode(ch, None, None, None, None, *widths, corr_factor=0.7, max_it=200, layers=g) for ch in CH]
        be = np.array([int(((r[0] < 0) != xi).sum()) for r, xi in zip(runs, x)])
        it = np.array([r[1] for r in runs])
        for min_errors, max_blocks in ((10 ** 9, 64), (2, 64), (10 ** 9, 23)):
            if min_errors == 2 and int((be > 0).sum()) < 2:
                continue
            r = consume_in_seed_order(be, it, c.N, min_errors, max_blocks)
            want = dict(ber=r["bit_errors"] / (r["blocks"] * c.N), blocks=r["blocks"], block_errors=r["block_errors"],
                        bit_errors=r["bit_errors"], nit_total=r["iters_total"])
            got = sp.sim_ldpc_mc(lp, sigma, MIN_ERRORS=min_errors, MAX_BLOCKS=max_blocks, batch=32, dectype=DT,
                                 quant=widths)
            assert got == want, (widths, min_errors, max_blocks, got, want)
        print(f"sim_ldpc_mc {widths}: {int((be > 0).sum())} failed of 64, {int(it.sum())} sweeps")
