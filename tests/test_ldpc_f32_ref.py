"""CPU: the NumPy statement of the binary32 layered decoders
(tests/ldpc_f32_ref.py) pinned to the binary64 statement
(tests/ldpc_layered_ref.py) where both are exact, its input clamp, and the
decoder names of the Python interface."""
import numpy as np
import pytest

import ldpc_cases as lc
import ldpc_f32_ref as fr
import ldpc_layered_ref as lr

DBL_MAX = float(np.finfo(np.float64).max)


@pytest.mark.parametrize("cell,sweeps", [("16_1/2_z24", 1), ("16_5/6_z24", 3), ("syn_dc32", 2)])
def test_minsum_on_dyadic_inputs_equals_the_binary64_statement(cell, sweeps):
    """Layered minsum with corr_factor = 0.5 on LLRs that are multiples of 2^-6 in [-8, 8]: subtract,
    add, min and a halving.  A layer's halving adds at most one bit below the last, so after s layer
    updates every quantity is a multiple of 2^-(6+s); while all of them stay under 2^(24-6-s) each
    operation is exact in binary32 (and in binary64), and the two statements must return identical
    app (signs of zero included) and sweep counts.  That holds for 12 layer updates at |.| < 64:
    one sweep of the 12 layers of 802.16 1/2, three of the 4 of 5/6, two of the synthetic graph's 5."""
    c = lc.make_code(cell)
    layers = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    steps = sweeps * (len(layers.first_check) - 1)
    assert steps <= 12
    rs = np.random.RandomState(11)
    seen = set()
    for w in range(6):
        x = lc._codeword(c, rs)
        ch = (1.0 - 2 * x) * 3.0 + rs.randn(c.N) * (0.5 + 0.4 * w)
        ch = np.clip(np.round(ch * 64.0) / 64.0, -8.0, 8.0)
        if w == 5:
            ch[:c.z] = 0.0
            ch[c.z:2 * c.z] = -0.0
        for k in range(sweeps + 1):
            a64, i64, t64, _ = lr.decode_code(c, ch, "minsum", corr_factor=0.5, max_it=k, trace=True, layers=layers)
            a32, i32, t32, _ = fr.decode_code(c, ch, "minsum", corr_factor=0.5, max_it=k, trace=True, layers=layers)
            assert i32 == i64
            if k:
                # |q| <= |app| + |r| and |r| <= |q| / 2 <= |app|: everything stays under 2 max |app| < 64
                assert np.abs(t64).max() < 32.0
                assert np.array_equal(t32, t64) and np.array_equal(np.signbit(t32), np.signbit(t64))
            assert np.array_equal(a32, a64) and np.array_equal(np.signbit(a32), np.signbit(a64))
        seen.add(i64)
    assert len(seen) > 1  # words that take different numbers of sweeps


def test_clamp_on_load():
    ch = np.array([DBL_MAX, -DBL_MAX, np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-50, -1e-50, 2.0 ** 100, 2.0 ** 101,
                   1.5, -3e38])
    c32 = fr.ch32(ch)
    assert c32.dtype == np.float32
    big = np.float32(2.0 ** 100)
    assert np.array_equal(c32[:4], [big, -big, big, -big])
    assert np.isnan(c32[4])
    assert np.array_equal(c32[5:9], [0, 0, 0, 0])
    assert np.array_equal(np.signbit(c32[5:9]), [False, True, False, True])  # 1e-50 rounds to a zero of its sign
    assert np.array_equal(c32[9:], [big, big, np.float32(1.5), -big])


@pytest.mark.parametrize("algo", fr.ALGOS)
def test_clamped_words_decode_without_nan(algo):
    """+-DBL_MAX and +-inf in ch come out as +-2^100 and stay finite through the sweeps; a NaN in ch
    reaches only the variables of its own checks; 1e-50 is an undecided zero until a sweep has run."""
    c = lc.make_code("16_1/2_z24")
    layers = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    x, ch = lc.awgn_word(c, 0.6, 0)
    sat = np.random.RandomState(3).permutation(c.N)[:8]
    ch[sat] = (1.0 - 2 * x[sat]) * np.array([DBL_MAX, np.inf] * 4)
    app, it = fr.decode_code(c, ch, algo, layers=layers)
    assert np.isfinite(app).all() and 0 < it < 200
    assert np.array_equal(np.abs(app[sat]), np.full(8, 2.0 ** 100))  # a float32 at 2^100 absorbs every message
    assert np.array_equal(app < 0, x == 1)
    # all of them against one check's other inputs: still finite (no inf - inf)
    app, it = fr.decode_code(c, np.where(x == 1, -np.inf, np.inf), algo, layers=layers)
    assert it == 0 and np.array_equal(app, np.where(x == 1, -1.0, 1.0) * 2.0 ** 100)
    wrong = np.where(x == 1, -np.inf, np.inf)
    wrong[::7] *= -1.0
    app, it = fr.decode_code(c, wrong, algo, max_it=6, layers=layers)
    assert np.isfinite(app).all() and 0 < it <= 6

    # the smallest denormal-to-zero input: undecided, so the word is not accepted at sweep 0
    tiny = 10.0 * (0.5 - x)
    tiny[5] = 1e-50
    app0, it0 = fr.decode_code(c, tiny, algo, max_it=0, layers=layers)
    assert it0 == 0 and app0[5] == 0.0
    app, it = fr.decode_code(c, tiny, algo, layers=layers)
    assert it == 1 and np.array_equal(app < 0, x == 1) and app[5] != 0.0

    # a NaN: it reaches a variable only through checks, layer after layer in the order of the sweep
    nan = ch.copy()
    nan[17] = np.nan
    app, it = fr.decode_code(c, nan, algo, max_it=1, layers=layers)
    assert it == 1 and np.isnan(app[17])
    touched = np.zeros(c.N, dtype=bool)
    touched[17] = True
    for k in range(c.Nc):  # the checks in layer order
        vs = layers.var_of[layers.cstart[k]:layers.cstart[k + 1]]
        if touched[vs].any():
            touched[vs] = True
    assert not touched.all() and not np.isnan(app[~touched]).any()
    if algo == "sumprod2":  # NaN + c(NaN) spreads to the whole check; minsum's fmin drops it
        assert np.isnan(app[touched]).all()


def test_sumprod2_is_the_binary64_decoder_rounded():
    """Not a bar, a sanity check of the statement: on a word that converges, the binary32 app agrees
    with the binary64 layered statement to binary32 accuracy and stops after the same sweeps."""
    c = lc.make_code("16_1/2_z24")
    ch = lc.awgn_word(c, 0.62, 0)[1]
    a64, i64 = lr.decode_code(c, ch, "sumprod2")
    for rounded in (False, True):
        a32, i32 = fr.decode_code(c, ch, "sumprod2", rounded=rounded)
        assert i32 == i64
        np.testing.assert_allclose(a32, a64, rtol=1e-4, atol=1e-4)


def test_decoder_names():
    from sparc_ldpc_amd import ldpc
    for name, base in (("layered_sumprod2_f32", "layered_sumprod2"), ("layered_minsum_f32", "layered_minsum")):
        assert name in ldpc._ALGOS and name not in ldpc._REFERENCE_ALGOS
        assert ldpc._ALGOS[name] == ldpc._ALGOS[base] | ldpc.LB_F32 and ldpc.LB_F32 == 0x100
    assert len(set(ldpc._ALGOS.values())) == len(ldpc._ALGOS) == 7
    c = ldpc.code("802.16", "1/2", 24)
    with pytest.raises(NameError, match="Decoder type unknonwn"):
        c.decode(np.ones(c.N), "layered_sumprod2_f32")
    with pytest.raises(ValueError):
        c.layer_info(precision="f16")
