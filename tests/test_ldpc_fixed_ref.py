"""The NumPy statement of fixed-point layered min-sum (tests/ldpc_fixed_ref.py),
on the CPU: where no clip fires it is binary64 layered min-sum bit for bit, its
rounding and saturation follow hand-computed vectors, its argument checks mirror
the library's ranges; and the Python entry points' ``quant`` keyword (no device
needed)."""
import numpy as np
import pytest

import ldpc_fixed_cases as qc
import ldpc_fixed_ref as qr
import ldpc_layered_cases as llc
import ldpc_layered_ref as lr

DBL_MAX = float(np.finfo(np.float64).max)


@pytest.mark.parametrize("cell", list(llc.CELLS))
def test_without_clips_the_statement_is_binary64_layered_minsum(cell):
    """All nine cells of the layered tests, both orders, widths (2, 8, 16), LLRs that are multiples of 2^-2
    in [-3, 3], 6 sweeps: app, sign of zero included, and the sweep counts equal ldpc_layered_ref's min-sum
    at corr_factor 1.  Precondition, from the statement: no clip fires."""
    c = llc.make_code(cell)
    g = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    CH = _pin(cell, c)
    assert np.array_equal(CH * 4, np.rint(CH * 4)) and np.abs(CH).max() <= 3.0 and not np.signbit(CH[CH == 0]).any()
    its = []
    for ch in CH:
        want, wit = lr.decode(ch, None, None, None, None, "minsum", corr_factor=1.0, max_it=qc.PIN_SWEEPS, layers=g)
        for order in ("layer", "check"):
            if order == "check" and c.Nc > 1200 and ch is not CH[0]:
                continue  # one check at a time on the large cells: one word keeps this test quick
            clips = {}
            app, it = qr.decode(ch, None, None, None, None, *qc.PIN_WIDTHS, corr_factor=1.0, max_it=qc.PIN_SWEEPS,
                                order=order, layers=g, clips=clips)
            assert sum(clips.values()) == 0, (order, clips)
            assert it == wit and np.array_equal(app, want) and np.array_equal(np.signbit(app), np.signbit(want))
        # and none fires at (3, 8, 16) either (the GPU tests' precondition for these words)
        clips = {}
        qr.decode(ch, None, None, None, None, 3, 8, 16, corr_factor=1.0, max_it=qc.PIN_SWEEPS, layers=g, clips=clips)
        assert sum(clips.values()) == 0, clips
        its.append(wit)
    assert max(its) == qc.PIN_SWEEPS  # some word is still running: six sweeps were compared


def _pin(cell, c):
    """qc.pin_words for the layered tests' cells (16_5/6_z300 included)."""
    rows = [ch for lab, ch in zip(*llc.words(cell, "minsum", c)) if lab == "awgn"]
    rows.append(3.0 * np.random.RandomState(0).randn(c.N))
    return np.clip(np.rint(np.array(rows) * 2.0) / 4.0, -3.0, 3.0) + 0.0


def test_pin_words_of_the_shared_cases_are_the_ones_compared_here():
    for cell in ("16_1/2_z24", "16_5/6_z192"):
        c = qc.make_code(cell)
        assert np.array_equal(qc.pin_words(cell, c), _pin(cell, c))


def test_channel_rounding_and_saturation():
    # F = 2: ch 2^F = +-0.5 and +-1.5 round half to even, to 0 and +-2
    ch = np.array([0.125, -0.125, 0.375, -0.375, 0.126, -0.124, 0.374, 0.625, -0.625])
    assert qr.quantise(ch, 2, 31).tolist() == [0, 0, 2, -2, 1, 0, 1, 2, -2]
    # NaN -> 0; +-inf and +-DBL_MAX -> +-rmax; -0.0 -> 0
    clips = {}
    q = qr.quantise(np.array([np.nan, np.inf, -np.inf, DBL_MAX, -DBL_MAX, -0.0, 0.0, 7.75, 8.0, -8.0]), 2, 31, clips)
    assert q.tolist() == [0, 31, -31, 31, -31, 0, 0, 31, 31, -31] and clips["channel"] == 6
    assert qr.quantise(np.array([0.49, 0.5, 1.5, 2.5, -2.5, 300.0]), 0, 1).tolist() == [0, 0, 1, 1, -1, 1]
    assert qr.quantise(np.array([1 / 256, 3 / 512, 1 / 512]), 8, 127).tolist() == [1, 2, 0]


def test_an_erased_or_nan_bit_leaves_its_checks_unsatisfied():
    cell = "16_1/2_z24"
    c = qc.make_code(cell)
    g = qc.layers(cell)
    import ldpc_cases as lc
    x = lc._codeword(c, np.random.RandomState(1))
    ch = 10.0 * (0.5 - x)
    app, it = qr.decode(ch, None, None, None, None, layers=g)
    assert it == 0 and np.array_equal(app, ch)  # +-5 = +-20 quarter-steps, under rmax
    for bad in (-0.0, np.nan, 0.1):  # 0.1 * 4 rounds to 0
        z = ch.copy()
        z[5] = bad
        app, it = qr.decode(z, None, None, None, None, layers=g)
        assert it >= 1 and np.array_equal(app < 0, x == 1) and not (app == 0).any()
        assert not np.signbit(qr.decode(z, None, None, None, None, layers=g, max_it=1, trace=True)[2][0][5])
    app, it = qr.decode(ch, None, None, None, None, layers=g, max_it=0)
    assert it == 0 and np.array_equal(app, ch)  # max_iter = 0: the channel itself, unquantised


def test_message_scaling_by_hand():
    rmax, amax = 31, 127  # (msg_bits, app_bits) = (6, 8)
    m = np.array([0, 1, 2, rmax, amax])
    want = {1: [0, 0, 0, 2, 8],  # (m + 8) >> 4
            11: [0, 1, 1, 21, 31],  # (11 m + 8) >> 4: 8, 19, 30, 349, 1405 -> 0, 1, 1, 21, 87 -> rmax
            12: [0, 1, 2, 23, 31],  # 8, 20, 32, 380, 1532 -> 0, 1, 2, 23, 95 -> rmax
            16: [0, 1, 2, 31, 31]}  # m, clipped
    for alpha, w in want.items():
        assert qr.scale(alpha, m, rmax).tolist() == w, alpha
    assert qr.parameters(2, 6, 8, 0.7) == (31, 127, 11)  # 11.2 -> 11
    assert qr.parameters(2, 6, 8, 0.71875)[2] == 12 and qr.parameters(2, 6, 8, 0.65625)[2] == 10  # 11.5, 10.5: to even
    # one check by hand, alpha 12: q = (5, -3, 9, -3): the two smallest tie at 3
    R = qr.check_rule(np.array([[5, -3, 9, -3]]), 12, rmax, amax)
    assert R.tolist() == [[2, -2, 2, -2]]  # mag 3 everywhere -> (36 + 8) >> 4 = 2; signs: the others' product
    R = qr.check_rule(np.array([[5, -2, 9, 4]]), 16, rmax, amax)
    assert R.tolist() == [[-2, 4, -2, -2]]
    assert qr.check_rule(np.array([[-6]]), 16, rmax, amax).tolist() == [[31]]  # no other edge: mag = amax -> rmax
    # the two orders agree, clips and all, where every clip fires
    cell = "16_1/2_z24"
    ref = qc.reference(cell, (1, 4, 6))
    assert all(ref.clips[k] > 0 for k in ("channel", "q", "r", "app"))
    for ch, it, apps in zip(ref.CH, ref.its, ref.apps):
        clips = {}
        app, it2, apps2 = qr.decode(ch, None, None, None, None, 1, 4, 6, corr_factor=0.75, max_it=qc.K_TRACE,
                                    order="check", trace=True, layers=ref.layers, clips=clips)
        assert it2 == it and np.array_equal(apps2, apps)


@pytest.mark.parametrize("cell", ["syn_dc8", "16_5/6_z24"])
def test_the_case_words_satisfy_their_preconditions(cell):
    """The whole table is asserted by the GPU tests; two small cells here."""
    qc.check_preconditions(cell)
    assert set(qc.CELLS) <= set(llc.CELLS)


def test_argument_checks_mirror_the_library():
    good = [(0, 2, 2), (8, 8, 16), (2, 6, 8), (3, 8, 8), (0, 2, 16)]
    bad = [(-1, 6, 8), (9, 6, 8), (2, 1, 8), (2, 9, 9), (2, 6, 5), (2, 6, 17), (2.5, 6, 8)]
    for w in good:
        qr.parameters(*w, 0.75)
    for w in bad:
        with pytest.raises(ValueError):
            qr.parameters(*w, 0.75)
    for corr in (1 / 32, 1.03, 0.0625, 1.0):  # alpha 0 -> rint(0.5) = 0: out; 16.48 -> 16; 1; 16
        if corr == 1 / 32:
            with pytest.raises(ValueError):
                qr.parameters(2, 6, 8, corr)
        else:
            assert 1 <= qr.parameters(2, 6, 8, corr)[2] <= 16
    for corr in (0.0, -0.75, 1.04, 2.0, float("nan"), float("inf")):  # 16.64 -> 17
        with pytest.raises(ValueError):
            qr.parameters(2, 6, 8, corr)


def test_quant_needs_layered_minsum_in_every_entry():
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc, ldpc_awgn, ldpc_bsc, ldpc_mc
    assert len(ldpc._ALGOS) == 7 and ldpc.LB_FIXED == 0x400 and ldpc.FIXED_DEFAULT == (2, 6, 8)
    assert ldpc._quant_widths(None, "sumprod2") is None and ldpc._quant_widths(True, "layered_minsum") == (2, 6, 8)
    assert ldpc._quant_widths([1, 4, 6], "layered_minsum") == (1, 4, 6)
    c = ldpc.code("802.16", "1/2", 24)
    lp = sp.LDPCParams("802.16", "1/2", 24)
    ch = np.zeros((1, c.N))
    for dectype in ("sumprod2", "minsum", "layered_sumprod2", "layered_minsum_f32", "layered_sumprod2_f32"):
        for quant in (True, (2, 6, 8)):
            calls = [
                lambda: c.decode_batch(ch, dectype, quant=quant),
                lambda: c.run_buffers(1, dectype, quant=quant),
                lambda: c.mc_blocks(None, ch, 0.8, dectype=dectype, quant=quant),
                lambda: c.mc_blocks_seeds([1], 0.8, dectype=dectype, quant=quant),
                lambda: ldpc_mc.mc_ldpc(c, 0.8, [1], dectype=dectype, quant=quant),
                lambda: sp.sim_ldpc_mc(lp, 0.8, MAX_BLOCKS=2, dectype=dectype, quant=quant),
                lambda: ldpc_awgn.sim("802.16", "1/2", 24, N_MEASUREMENTS=1, MAX_BLOCKS=2, dectype=dectype, quant=quant),
                lambda: ldpc_bsc.sim("802.16", "1/2", 24, repeats=1, dectype=dectype, quant=quant),
            ]
            if dectype.startswith("layered_"):  # (a flooding type with stream=True is refused first, as ever)
                calls.append(lambda: c.mc_stream_seeds([1], 0.8, dectype=dectype, quant=quant))
                calls.append(lambda: ldpc_mc.mc_ldpc(c, 0.8, [1], dectype=dectype, draws="device", stream=True,
                                                     quant=quant))
            for call in calls:
                with pytest.raises(ValueError, match="layered_minsum"):
                    call()
    assert c._ctx is None  # none of them reached the library
    for quant in (3, (2, 6), (2, 6, 8, 8), (2, 6, "x")):
        with pytest.raises(ValueError, match="quant must be"):
            c.decode_batch(ch, "layered_minsum", quant=quant)
    assert c._ctx is None
    with pytest.raises(TypeError):
        c.decode(ch[0], "minsum", 0.7, quant=True)  # the reference's signature does not take it
