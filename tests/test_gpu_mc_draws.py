"""GPU: Monte-Carlo reps drawn on the device from their seeds (sa_mc_draw,
csrc/legacy_mt_dev.h) — NumPy's legacy generator run by one workgroup per rep —
against NumPy itself (harness._draw_reps), and the rep stream on such draws
against the stream on the same arrays staged from the host.

The noise bar, 2**-49 relative, is derived, not tuned: the device library's
log and the C library's are each within 1 ulp of the true value, so they differ
by <= 2 * 2**-52; the division, the square root, the product with x and the
product with sigma add at most half an ulp each on either side, and the square
root halves what is in front of it: <= 4.5 * 2**-52 < 2**-49.  A misaligned
accept sequence shows as differences of order 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 2.0 ** -49
# 0, 1, the top bit, the largest seed, and consecutive ones: 11 reps (one workgroup each)
SEEDS = [0, 1, 2 ** 31, 2 ** 32 - 1] + list(range(1000, 1007))
SIGMAS = 0.3 + 0.07 * np.arange(len(SEEDS))

# (L, M, n): where the generator can go wrong, not the workload's shape
SHAPES = [
    (3, 8, 1),          # one value, its cached partner dropped, no second twist
    (5, 4, 7),          # L % 4 != 0: the trials are misaligned to the 624-word block
    (63, 64, 4607),     # misaligned, odd n, about 19 twists with straddling trials
    (128, 256, 1024),   # aligned
]


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


def _op(sp, L, M, n, prec="fp32"):
    return sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=prec)


def _numpy_reps(sp, seeds, L, M, n, sigmas):
    from sparc_ldpc_amd.harness import _draw_reps
    idx = np.empty((len(seeds), L), dtype=np.int32)
    noise = np.empty((len(seeds), n))
    for i, (s, sg) in enumerate(zip(seeds, sigmas)):
        ix, nz = _draw_reps([s], L, M, n, sg)
        idx[i], noise[i] = ix[0], nz[0]
    return idx, noise


@pytest.mark.parametrize("L,M,n", SHAPES)
def test_device_draws_against_numpy(sp, L, M, n):
    op = _op(sp, L, M, n)
    ms = op.mc_draw(SEEDS, SIGMAS)
    idx, noise = op.mc_fetch_draws()
    ref_idx, ref_noise = _numpy_reps(sp, SEEDS, L, M, n, SIGMAS)
    assert idx.shape == ref_idx.shape and noise.shape == ref_noise.shape
    np.testing.assert_array_equal(idx, ref_idx)
    zero = ref_noise == 0
    ratio = np.abs(noise - ref_noise)[~zero] / np.abs(ref_noise[~zero])
    differ = int((noise != ref_noise).sum())
    print(f"L={L} M={M} n={n}: draw {ms:.3f} ms, {differ} of {noise.size} values differ "
          f"({100.0 * differ / noise.size:.3f} %), largest ratio {ratio.max() * 2.0 ** 52:.3f} * 2**-52")
    assert np.all(noise[zero] == 0)
    assert np.all(np.isfinite(noise))
    assert ratio.max() <= BAR


@pytest.mark.parametrize("prec,B,nreps,T", [("fp32", 8, 37, 12), ("fp64", 8, 30, 25)])
def test_stream_on_device_draws_is_the_stream(sp, prec, B, nreps, T):
    """L=128 M=256 R=1 (test_stream_edge_cases' shape), two sigmas interleaved
    in one stream: mc_stream_seeds against mc_stream on the arrays
    mc_fetch_draws returned, on one operator with nreps, then fewer, then more
    reps (the cached stream graphs, re-staging within and past the capacity)."""
    L, M = 128, 256
    op = _op(sp, L, M, L * 8, prec)
    assert op.mc_supported(B)
    Pl = 2.0 / L * np.ones(L)
    for rnd, R in enumerate((nreps, 13, nreps + 16)):
        seeds = list(range(500 + 100 * rnd, 500 + 100 * rnd + R))
        sig = np.where(np.arange(R) % 2 == 0, 0.55, 0.7)
        tm = {}
        be, it, ms = sp.mc_stream_seeds(op, Pl, T, seeds, sig, batch=B, timings=tm)
        assert ms > 0 and tm["draw_ms"] > 0
        idx, noise = op.mc_fetch_draws()
        assert idx.shape == (R, L) and noise.shape == (R, op.n)
        be0, it0, _ = sp.mc_stream(op, Pl, T, idx, noise, batch=B)
        np.testing.assert_array_equal(be, be0, err_msg=f"bit errors, round {rnd}")
        np.testing.assert_array_equal(it, it0, err_msg=f"stop index, round {rnd}")
        assert be.dtype == np.int64 and len(be) == R
        assert it.min() >= 0 and it.max() <= T


def test_mc_decode_device_draws(sp):
    """mc_decode(draws="device") is the stream on device draws; a rep whose
    device-drawn noise equals the host-drawn noise bit for bit has the result of
    mc_decode(draws="host").  (The other reps' noise differs in a last bit
    somewhere: their results are not compared; their number is printed.)"""
    L, M, T, B = 128, 256, 12, 8
    op = _op(sp, L, M, L * 8)
    Pl = 2.0 / L * np.ones(L)
    seeds = list(range(500, 537))
    sg = 0.55
    be, it = sp.mc_decode(op, Pl, sg, T, seeds, batch=B, draws="device")
    idx, noise = op.mc_fetch_draws()
    be_s, it_s, _ = sp.mc_stream_seeds(op, Pl, T, seeds, sg, batch=B)
    np.testing.assert_array_equal(be, be_s)
    np.testing.assert_array_equal(it, it_s)
    be_h, it_h = sp.mc_decode(op, Pl, sg, T, seeds, batch=B, draws="host")
    idx_h, noise_h = sp.draw_reps(seeds, L, M, op.n, sg)
    np.testing.assert_array_equal(idx, idx_h)
    same = np.all(noise == noise_h, axis=1)
    print(f"{int((~same).sum())} of {len(seeds)} reps hold a noise value that differs from the host draw")
    print(f"{int(((be != be_h) | (it != it_h)).sum())} of {len(seeds)} reps have another result than on host draws")
    np.testing.assert_array_equal(be[same], be_h[same])
    np.testing.assert_array_equal(it[same], it_h[same])
    # default: host draws, as before
    be_d, it_d = sp.mc_decode(op, Pl, sg, T, seeds, batch=B)
    np.testing.assert_array_equal(be_d, be_h)
    np.testing.assert_array_equal(it_d, it_h)


def test_device_draw_refusals(sp):
    from sparc_ldpc_amd import _lib
    L, M = 32, 64
    n = L * 6
    op = _op(sp, L, M, n)
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
            op.mc_draw([1, bad, 3], 0.5)
    with pytest.raises((AssertionError, sp.SparcAmpError)):  # SA_ERR_ARG raises AssertionError
        op.mc_draw([], 0.5)                                   # nreps = 0
    with pytest.raises((AssertionError, sp.SparcAmpError)):
        op.mc_fetch_draws()                                   # nothing staged
    # M = 100: randint(0, 100) rejects draws, the device generator does not
    n100 = int(8 * np.log2(100))
    op100 = _op(sp, 8, 100, n100)
    with pytest.raises(sp.SparcAmpError) as ei:
        op100.mc_draw([1, 2, 3], 0.5)
    assert ei.value.code == _lib.SA_ERR_UNSUPPORTED
    # a drawn stream still needs its power allocation
    op.mc_draw([1, 2, 3], 0.5)
    with pytest.raises((AssertionError, sp.SparcAmpError)):
        op.mc_run(8, 10)
