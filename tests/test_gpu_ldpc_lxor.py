"""GPU: the check-node rules of libldpc_bp.so on their own.  Lxor (with the
decoder's own logarithm, log12) against Lxor in long double at every edge of
its arithmetic; Lxfb at every check degree against the NumPy oracle."""
import numpy as np
import pytest

import ldpc_cases as lc
from oracle import ldpc_oracle as lo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def code():
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible: -m gpu tests need an MI355X"
    return ldpc.code("802.16", "1/2", 3)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def test_lxor_against_long_double(code):
    """|device - lxor_ld| <= 4 * 2^-52 * max(1, min(|a|, |b|)) (derivation: ldpc_cases.lxor_bar)."""
    a, b = lc.lxor_points()
    got = np.array([code.Lxor(x, y, 1) for x, y in zip(a, b)])
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.longdouble) - lo.lxor_ld(a, b)).astype(np.float64)
    units = err / lc.lxor_bar(a, b) * 4
    i = int(np.argmax(units))
    print(f"\nLxor: {len(a)} points, worst error {units[i]:.3f} * 2^-52 * max(1, min(|a|, |b|)) "
          f"at a={float(a[i])!r} b={float(b[i])!r}")
    assert np.all(err <= lc.lxor_bar(a, b)), (units[i], a[i], b[i])


def test_lxor_zeros_and_uncorrected_rule_bit_exact(code):
    """A zero of either sign on either side, and corr = 0 everywhere: the float64 oracle's bits
    (sign * min has no rounding; Lxor(a, +-0) = +-0 + t - t with the same t twice)."""
    a, b = lc.lxor_points()
    z = (a == 0) | (b == 0)
    assert z.sum() >= 40 and (np.signbit(a[z]) & (a[z] == 0)).any() and (~np.signbit(b[z]) & (b[z] == 0)).any()
    got = np.array([code.Lxor(x, y, 1) for x, y in zip(a[z], b[z])])
    assert np.array_equal(_bits(got), _bits(lo.lxor(a[z], b[z], True)))
    sel = np.concatenate([np.nonzero(z)[0], np.arange(0, len(a), 7)])
    got = np.array([code.Lxor(x, y, 0) for x, y in zip(a[sel], b[sel])])
    assert np.array_equal(_bits(got), _bits(lo.lxor(a[sel], b[sel], False)))


@pytest.mark.parametrize("corr", [0, 1])
def test_lxfb_every_degree(code, corr):
    """Lxfb at dc = 2..32 (dc = 1 reads b[1] in the reference: out of range there), three input
    scales; corr = 0 is sign * min only: bit-exact."""
    rs = np.random.RandomState(31)
    for dc in range(2, 33):
        for scale in (0.3, 3.0, 30.0):
            L = rs.randn(dc) * scale
            agg, out = code.Lxfb(L, corr)
            Lm = L[None, :].copy()
            agg_o = lo.lxfb(Lm, bool(corr))
            if corr:
                np.testing.assert_allclose(out, Lm[0], rtol=1e-13, atol=1e-14, err_msg=f"dc={dc} scale={scale}")
                assert abs(agg - agg_o[0]) <= 1e-13 * max(1.0, abs(agg)), (dc, scale)
            else:
                assert np.array_equal(_bits(out), _bits(Lm[0])) and _bits(agg) == _bits(agg_o[0]), (dc, scale)
