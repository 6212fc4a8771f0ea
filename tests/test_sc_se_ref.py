"""CPU: the NumPy statement of coupled state evolution (tests/sc_se_ref.py)
pinned to the uncoupled statement (tests/se_ref.py) where the two must agree,
and to its own definitions.

Bars: the project's convention, se_cases.TOL_FACTOR x the case's
binary64-against-longdouble gap, absolute; the gap is measured here from the
two statements (the larger of the coupled and the uncoupled one's)."""
import numpy as np
import pytest

import sc_ref
import sc_se_cases as scc
import sc_se_ref
import se_cases
import se_ref
from sc_cases import FLAT, FLAT_W

S, T = 33, 8


def _flat():
    L, M, n, P, sigma = FLAT["L"], FLAT["M"], FLAT["n"], FLAT["P"], FLAT["sigma"]
    return L, M, n, sigma, P / L * np.ones(L), se_cases.rows_of(FLAT["seed"], S, M)


def _gap(coupled, coupled_ld, flat, flat_ld):
    return max(float(np.max(np.abs(coupled[0] - coupled_ld[0]))), float(np.max(np.abs(coupled[2] - coupled_ld[2]))),
               float(np.max(np.abs(flat[0] - flat_ld[0]))), float(np.max(np.abs(flat[1] - flat_ld[1]))))


@pytest.mark.parametrize("name", sorted(FLAT_W))
def test_flat_base_matrix_is_the_uncoupled_statement(name):
    L, M, n, sigma, Pl, U = _flat()
    W = FLAT_W[name]
    R, C = W.shape
    r = sc_se_ref.sc_se_ref(Pl, sigma, M, n, W, T, U)
    r_ld = sc_se_ref.sc_se_ref(Pl, sigma, M, n, W, T, U, longdouble=True)
    f = se_ref.se_ref(Pl, sigma, M, n, T, U)
    f_ld = se_ref.se_ref(Pl, sigma, M, n, T, U, longdouble=True)
    tol = se_cases.TOL_FACTOR * _gap(r, r_ld, f, f_ld)
    phi, tau2, x, miss, E, stop = r
    assert phi.shape == (T + 1, R) and tau2.shape == (T, C) and x.shape == (T, C) and miss.shape == (T, C)
    d_phi = float(np.max(np.abs(phi - f[0][0][:, None])))
    d_tau = float(np.max(np.abs(tau2 - f[0][0][:T, None])))
    # every column block holds the same powers: the allocation's x is each block's x
    d_x = float(np.max(np.abs(x - f[1][0][:, None])))
    d_E = float(np.max(np.abs(E - f[3][0])))
    print(f"{name}: tol {tol:.3e}; phi {d_phi:.3e}, tau2 {d_tau:.3e}, x {d_x:.3e}, E {d_E:.3e}")
    assert max(d_phi, d_tau, d_x, d_E) <= tol
    np.testing.assert_array_equal(miss.sum(axis=1), f[2][0])


@pytest.mark.parametrize("Lambda", [2, 4])
def test_omega_1_decouples(Lambda):
    """base_matrix(1, Lambda) = Lambda I: block c sees rows n/Lambda of power
    Lambda Pl alone, with c_l unchanged and tau_c^2 = phi_c."""
    L, M, n, sigma = 16, 16, 64, 0.5
    U = se_cases.rows_of(3, S, M)
    Lc = L // Lambda
    powers = 2.0 * (1.0 + 0.25 * np.arange(Lambda)) / Lambda  # a different power in each column block
    Pl = np.repeat(powers / Lc, Lc)
    W = sc_ref.base_matrix(1, Lambda)
    np.testing.assert_array_equal(W, Lambda * np.eye(Lambda))
    r = sc_se_ref.sc_se_ref(Pl, sigma, M, n, W, T, U)
    r_ld = sc_se_ref.sc_se_ref(Pl, sigma, M, n, W, T, U, longdouble=True)
    for c in range(Lambda):
        blk = Lambda * Pl[c * Lc:(c + 1) * Lc]
        f = se_ref.se_ref(blk, sigma, M, n // Lambda, T, U)
        f_ld = se_ref.se_ref(blk, sigma, M, n // Lambda, T, U, longdouble=True)
        tol = se_cases.TOL_FACTOR * _gap(r, r_ld, f, f_ld)
        d_phi = float(np.max(np.abs(r[0][:, c] - f[0][0])))
        d_tau = float(np.max(np.abs(r[1][:, c] - f[0][0][:T])))
        d_x = float(np.max(np.abs(r[2][:, c] - f[1][0])))
        d_E = float(np.max(np.abs(r[4][c * Lc:(c + 1) * Lc] - f[3][0])))
        print(f"Lambda {Lambda}, block {c}: tol {tol:.3e}; phi {d_phi:.3e}, tau2 {d_tau:.3e}, x {d_x:.3e}, E {d_E:.3e}")
        assert max(d_phi, d_tau, d_x, d_E) <= tol
        np.testing.assert_array_equal(r[3][:, c], f[2][0])


@pytest.mark.parametrize("name", list(scc.CASES))
def test_phi_0_and_the_stop_index(name):
    c = scc.case(name)
    assert c.margin >= scc.MARGIN
    for b in range(c.B):
        W, Pl, R, C = c.W[b], c.Pl[b], c.R[b], c.C[b]
        Pc = [0.0] * C
        for l in range(c.L):  # P_c in section order
            Pc[l // (c.L // C)] += Pl[l]
        sig2 = c.sigma[b] * c.sigma[b]
        for r in range(R):  # phi^0 = sigma^2 + W P_c exactly, c in order
            acc = 0.0
            for k in range(C):
                acc += W[r, k] * Pc[k]
            assert c.phi[b][0, r] == sig2 + acc
        # the stop index: the first bit-repeat of the phi row, or T
        rep = [t for t in range(1, c.T + 1) if c.phi[b][t].tobytes() == c.phi[b][t - 1].tobytes()]
        assert c.stop[b] == (rep[0] if rep else c.T)
        # the two precisions agree on it and on the miss counts (scripts/sc_se_case_seeds.py)
        ld = sc_se_ref.sc_se_ref(Pl, c.sigma[b], c.M, c.n[b], W, c.T, c.U, longdouble=True)
        assert ld[5] == c.stop[b]
        np.testing.assert_array_equal(ld[3], c.miss[b])
        gap = max(float(np.max(np.abs(a - d))) for a, d in ((c.phi[b], ld[0]), (c.tau2[b], ld[1]), (c.x[b], ld[2]),
                                                             (c.E[b], ld[4])))
        assert gap <= c.gap  # the recorded gap is the case's largest


def test_the_cases_cover_what_they_name():
    assert scc.case("band_2_4").stop[0] < scc.case("band_2_4").T - 8  # T far past convergence
    c = scc.case("pa_blocks")
    blocks = c.Pl[0].reshape(c.C[0], -1)
    assert any(len(set(blk.tolist())) > 1 for blk in blocks)  # several classes a block
    assert set(blocks[-1].tolist()) == set(blocks[-2].tolist()) and len(set(blocks[-1].tolist())) == 1  # one power, two blocks
    assert c.M & (c.M - 1)
    c = scc.case("general_W")
    assert c.R[0] < c.C[0] and (c.W[0] == 0).any()
    assert (scc.case("rows_64").R[0], scc.case("rows_64").C[0]) == (scc.MAX_BLOCKS, 61)
    assert (scc.case("square_64").R[0], scc.case("square_64").C[0]) == (scc.MAX_BLOCKS, scc.MAX_BLOCKS)
    c = scc.case("batch_mixed")
    assert len(set(c.R)) == 3 and len(set(c.C)) == 3 and len(set(c.sigma.tolist())) == 3 and len(set(c.n)) == 2
    assert len(set(c.Pl[2].tolist())) >= 5
    assert scc.case("max_M").M == scc.MAX_M
