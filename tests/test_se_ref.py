"""CPU: the NumPy statement of state evolution (tests/se_ref.py) pinned to the
reference's own denoiser, to closed forms and to its limits; the cases' recorded
seeds and gaps (tests/se_cases.py) against the statement; and the iterative
power allocation (harness.pa_iterative)."""
import numpy as np
import pytest

import se_cases as sc
import se_ref
from oracle import amp_oracle as orc


def test_posterior_is_the_reference_denoiser():
    """One iteration of the oracle's amp() on s = c e_true + tau U stacked over
    the sections: beta[true column] / c_l is the statement's per-sample
    posterior (the same formula, another summation order)."""
    L, M, n, tau = 6, 32, 16, 1.5
    Pl = orc.pa_parameterised(L, 1.2, 2.0, 1.0, 0.6)
    c = np.sqrt(n * Pl)
    U = np.random.RandomState(3).randn(5, M)
    y = tau * np.ones((n, 1))  # sum y^2 / n = tau^2 exactly
    assert np.sqrt(np.sum(y ** 2) / n) == tau
    for s in range(U.shape[0]):
        e_true = np.zeros(M)
        e_true[0] = 1.0
        stacked = np.concatenate([c[l] * e_true + tau * U[s] for l in range(L)]).reshape(-1, 1)
        beta = orc.amp(y, 0.0, Pl, L, M, 1, lambda b: np.zeros((n, 1)), lambda z: stacked)
        got = beta.reshape(L, M)[:, 0] / c
        want = np.array([se_ref.posterior(c[l] / tau, U[s:s + 1])[0][0] for l in range(L)])
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def test_two_columns_one_sample_closed_form():
    n, P, sigma = 1, 1.0, 0.7
    U = np.array([[0.3, -1.1]])
    tau2, x, miss, E = se_ref.se_ref([[P]], sigma, 2, n, 1, U)
    a = np.sqrt(n * P) / np.sqrt(sigma ** 2 + P)
    want = 1.0 / (1.0 + np.exp(a * (U[0, 1] - U[0, 0]) - a * a))
    np.testing.assert_allclose(x[0, 0], want, rtol=1e-15)
    np.testing.assert_allclose(E[0, 0], want, rtol=1e-15)
    np.testing.assert_allclose(tau2[0], [sigma ** 2 + P, sigma ** 2 + P * (1 - want)], rtol=1e-15)
    assert miss[0, 0] == int(a * a + a * U[0, 0] < a * U[0, 1])
    # and a row on which the true column loses
    _, _, miss, _ = se_ref.se_ref([[P]], sigma, 2, n, 1, np.array([[-2.0, 1.5]]))
    assert miss[0, 0] == 1


def test_uniform_allocation_is_one_section_of_weight_one():
    L, M, P, sigma, T = 12, 16, 2.0, 0.6, 6
    n = int(L * np.log2(M))
    U = np.random.RandomState(11).randn(40, M)
    t_u, x_u, m_u, E_u = se_ref.se_ref(P / L * np.ones((1, L)), sigma, M, n, T, U)
    # one section of power P over n / L rows: the same c = sqrt(n P / L), weight 1
    t_1, x_1, m_1, E_1 = se_ref.se_ref([[P]], sigma, M, n / L, T, U)
    np.testing.assert_allclose(t_u, t_1, rtol=1e-13)
    np.testing.assert_allclose(x_u, x_1, rtol=1e-13)
    np.testing.assert_array_equal(m_u, L * m_1)
    np.testing.assert_allclose(E_u, np.repeat(E_1, L, axis=1), rtol=1e-13)


def test_high_snr_limit():
    L, M, P, sigma, T = 4, 8, 2.0, 0.1, 4
    U = np.random.RandomState(2).randn(64, M)
    tau2, x, miss, E = se_ref.se_ref(P / L * np.ones((1, L)), sigma, M, 400, T, U)
    assert 1.0 - x[0, -1] < 1e-12
    assert abs(tau2[0, -1] - sigma ** 2) < 1e-11
    assert miss[0, -1] == 0


def test_longdouble_switch():
    U = np.random.RandomState(5).randn(9, 7)
    Pl = np.array([[0.5, 0.3, 0.2]])
    a = se_ref.se_ref(Pl, 0.5, 7, 12, 3, U)
    b = se_ref.se_ref(Pl, 0.5, 7, 12, 3, U, longdouble=True)
    assert b[0].dtype == np.longdouble and a[0].dtype == np.float64
    np.testing.assert_allclose(a[0], b[0].astype(np.float64), rtol=1e-13)
    np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("name", [k for k in sc.CASES if k != "batch3"])
def test_recorded_seed_and_gap(name):
    """The recorded choice is what scripts/se_case_seeds.py finds: no earlier
    seed qualifies and the recorded one does; the statement in np.longdouble
    lies within the tolerance the GPU tests take from the recorded gap."""
    seed, gap = sc._CHOSEN[name]
    for s in range(seed):
        assert sc.statement(name, s, margin=True)[4] < sc.MARGIN
    t2, x, _, _, margin = sc.statement(name, seed, margin=True)
    assert margin >= sc.MARGIN
    t2l, xl, _, _ = sc.statement(name, seed, longdouble=True)
    got = max(float(np.max(np.abs(t2 - t2l))), float(np.max(np.abs(x - xl))))
    assert 0 < gap and got <= sc.TOL_FACTOR * gap


def test_case_table():
    for name in sc.CASES:
        L, M, R, P, sigmas, S, T, allocs = sc.CASES[name]
        Pl, sig = sc.allocations(name)
        assert Pl.shape == (len(allocs), L) and sig.shape == (len(allocs),)
        np.testing.assert_allclose(Pl.sum(axis=1), P, rtol=1e-14)
        assert name in sc._CHOSEN
    assert len(np.unique(sc.allocations("distinct")[0])) == 5
    assert sc.CASES["max_M"][1] == sc.MAX_M


# ---- pa_iterative ---------------------------------------------------------------

def test_pa_iterative_sums_to_P_and_does_not_increase():
    from sparc_ldpc_amd import pa_iterative
    for L, B, sigma, P, R_PA in [(512, 512, 1.0, 3.0, 1.0), (512, 32, 1.1247, 4.0, 1.1), (40, 8, 0.5, 2.0, 0.9),
                                 (16, 16, 1.0, 15.0, 1.5), (12, 5, 1.0, 2.0, 1.0)]:
        pa = pa_iterative(L, B, sigma, P, R_PA)
        assert pa.shape == (L,)
        np.testing.assert_allclose(pa.sum(), P, rtol=1e-13)
        assert np.all(np.diff(pa) <= 0) and np.all(pa > 0)


def test_pa_iterative_one_block_is_uniform():
    from sparc_ldpc_amd import pa_iterative
    np.testing.assert_array_equal(pa_iterative(8, 1, 0.5, 2.0, 1.0), 2.0 / 8 * np.ones(8))
    np.testing.assert_array_equal(pa_iterative(8, 1, 0.5, 2.0, 5.0), 2.0 / 8 * np.ones(8))


def test_pa_iterative_by_hand():
    """L = 4, B = 2, sigma = 1, P = 3, R_PA = 0.8: k = 2 ln2 R_PA / L = 0.277259.
    Block 0: the rule gives 0.277259 * (1 + 3) = 1.109035 > 3 / 4, so sections
    0 and 1 get 1.109035 each and 3 - 2.218071 = 0.781929 is left.  Block 1 is
    the last: sections 2 and 3 share it evenly, 0.390965 each."""
    from sparc_ldpc_amd import pa_iterative
    k = 2 * np.log(2) * 0.8 / 4
    first = k * (1.0 + 3.0)
    rest = (3.0 - 2 * first) / 2
    np.testing.assert_allclose(pa_iterative(4, 2, 1.0, 3.0, 0.8), [first, first, rest, rest], rtol=1e-15)
    np.testing.assert_allclose(pa_iterative(4, 2, 1.0, 3.0, 0.8), [1.109035, 1.109035, 0.390965, 0.390965], atol=1e-6)


def test_pa_iterative_flat_tail_starts_where_the_rule_says():
    from sparc_ldpc_amd import pa_iterative
    L, B, sigma, P, R_PA = 24, 12, 0.8, 2.5, 1.0
    per = L // B
    pa = pa_iterative(L, B, sigma, P, R_PA)
    k = 2 * np.log(2) * R_PA / L
    left, start = P, None
    for blk in range(B):  # the rule, block by block
        need, even = k * (sigma ** 2 + left), left / (L - per * blk)
        if need <= even:
            start = per * blk
            break
        np.testing.assert_allclose(pa[per * blk:per * (blk + 1)], need, rtol=1e-13)
        left -= per * need
    assert start is not None and 0 < start < L - per  # a tail of several blocks, after some ruled ones
    np.testing.assert_allclose(pa[start:], left / (L - start), rtol=1e-13)
    assert len(np.unique(pa[start:])) == 1 and pa[start - 1] > pa[start]
