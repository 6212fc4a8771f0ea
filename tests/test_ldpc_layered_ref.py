"""The NumPy reference of the layered schedule (tests/ldpc_layered_ref.py), on
the CPU: its two evaluation orders agree bit for bit, it decodes, it never
needs more sweeps than the flooding oracle needs iterations on these words, and
its edge cases (max_iter = 0, erased bits, a layering that is none)."""
import numpy as np
import pytest

import ldpc_cases as lc
import ldpc_layered_cases as llc
import ldpc_layered_ref as lr
from oracle import ldpc_oracle as lo

CELLS = ("16_1/2_z24", "syn_dc8")
SIGMA = {"16_1/2_z24": 0.7, "syn_dc8": 0.6}  # where these short codes still decode every seed used


def _awgn(cell, n=4):
    c = lc.make_code(cell)
    return c, [lc.awgn_word(c, SIGMA[cell], seed) for seed in range(n)]


@pytest.mark.parametrize("algo", lr.ALGOS)
@pytest.mark.parametrize("cell", CELLS)
def test_per_check_and_per_layer_orders_agree_bit_for_bit(cell, algo):
    c, sent = _awgn(cell)
    assert cell != "syn_dc8" or (c.cdeg.min(), c.cdeg.max(), c.z) == (2, 8, 8)
    rows = [ch for _, ch in sent]
    rows += [lc.hopeless_word(c, 0.12, 0), 3.0 * np.random.RandomState(0).randn(c.N), lc.erase_word(c, 0.6, 0),
             lc.sat_word(c, 0)]
    layers = lr.Layers(c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c))
    for ch in rows:
        a, ia, ta, ma = lr.decode_code(c, ch, algo, max_it=8, order="layer", trace=True, layers=layers)
        b, ib, tb, mb = lr.decode_code(c, ch, algo, max_it=8, order="check", trace=True, layers=layers)
        assert ia == ib
        for x, y in ((a, b), (ta, tb), (ma, mb)):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(np.signbit(x), np.signbit(y))


@pytest.mark.parametrize("algo", lr.ALGOS)
@pytest.mark.parametrize("cell", CELLS)
def test_awgn_words_decode_in_no_more_sweeps_than_flooding_iterations(cell, algo):
    c, sent = _awgn(cell, 6)
    for x, ch in sent:
        app, it = lr.decode_code(c, ch, algo)
        assert it < lo.MAX_ITCOUNT
        hard = (app < 0).astype(np.int64)
        assert np.array_equal(hard, x)
        assert not (lo.pcmat(c.proto, c.z) @ hard % 2).any()  # a codeword
        _, fit = lo._decode(ch, c.vdeg, c.cdeg, c.intrlv, algo)
        assert it <= fit, (it, fit)


@pytest.mark.parametrize("algo", lr.ALGOS)
def test_max_iter_zero_and_truncation(algo):
    c, sent = _awgn("16_1/2_z24", 1)
    ch = sent[0][1]
    app, it = lr.decode_code(c, ch, algo, max_it=0)
    assert it == 0 and np.array_equal(app, ch)
    # a codeword already: 0 sweeps whatever max_iter
    x = sent[0][0]
    app, it = lr.decode_code(c, 10.0 * (0.5 - x), algo)
    assert it == 0 and np.array_equal(app, 10.0 * (0.5 - x))
    # the traced run cut at k is the run with max_iter = k
    _, full, apps, _ = lr.decode_code(c, ch, algo, max_it=12, trace=True)
    assert 1 < full < 12
    for k in range(0, 13):
        a, i = lr.decode_code(c, ch, algo, max_it=k)
        ta, ti = lr.truncated(full, apps, k)
        assert i == ti == min(k, full) and np.array_equal(a, ta)


@pytest.mark.parametrize("algo", lr.ALGOS)
def test_an_erased_word_does_not_stop_at_zero(algo):
    c = lc.make_code("16_1/2_z24")
    # the received signs form a codeword, but 2z bits are erased (+0.0 and -0.0)
    x = lc._codeword(c, np.random.RandomState(1))
    ch = 10.0 * (0.5 - x)
    assert lr.decode_code(c, ch, algo)[1] == 0
    ch[c.z:2 * c.z] = 0.0
    ch[c.N - 2 * c.z:c.N - c.z] = -0.0
    app, it = lr.decode_code(c, ch, algo)
    assert it > 0 and np.array_equal(app < 0, x == 1) and not (app == 0).any()
    assert lr.decode_code(c, lc.erase_word(c, 0.6, 0), algo)[1] > 0
    nan = 10.0 * (0.5 - x)
    nan[5] = np.nan
    assert lr.decode_code(c, nan, algo, max_it=3)[1] == 3  # a NaN never decides


def test_a_layering_with_a_repeated_variable_is_rejected():
    c = lc.make_code("16_1/2_z24")
    ch = lc.awgn_word(c, 0.7, 0)[1]
    fc = lr.code_layers(c)
    merged = np.delete(fc, 1)  # protograph rows 0 and 1 as one layer: they share columns
    with pytest.raises(AssertionError, match="occurs twice"):
        lr.decode(ch, c.vdeg, c.cdeg, c.intrlv, merged)
    for bad in (fc[:-1], np.concatenate([fc[:2], fc[1:]]), fc[1:]):
        with pytest.raises(AssertionError, match="increase strictly"):
            lr.decode(ch, c.vdeg, c.cdeg, c.intrlv, bad)
    # any split of the protograph rows is still a layering, with the same result as itself in both orders
    split = np.unique(np.concatenate([fc, fc[:-1] + c.z // 2]))
    a, ia = lr.decode(ch, c.vdeg, c.cdeg, c.intrlv, split, order="layer")
    b, ib = lr.decode(ch, c.vdeg, c.cdeg, c.intrlv, split, order="check")
    assert ia == ib and np.array_equal(a, b)


def test_lxfb_with_the_oracles_lxor_is_the_oracles_lxfb():
    rs = np.random.RandomState(3)
    for dc in (2, 3, 7, 20, 32):
        Lm = rs.randn(40, dc) * 4
        a, b = Lm.copy(), Lm.copy()
        ra = lo.lxfb(a, True)
        rb = lr._lxfb_with(b, True, lo.lxor)
        assert np.array_equal(a, b) and np.array_equal(ra, rb)
        c = Lm.copy()
        lr._lxfb_with(c, True, lr.lxor_log1p)
        np.testing.assert_allclose(c, a, rtol=1e-12, atol=1e-12)


def test_the_case_seeds_satisfy_their_preconditions_on_a_small_cell():
    """The whole table is asserted by the GPU tests; one small cell here."""
    for algo in llc.ALGOS:
        llc.reference("syn_dc8", algo).check_preconditions("syn_dc8", algo)
    assert set(llc.SEEDS) == set(llc.CELLS)
