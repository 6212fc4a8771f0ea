"""CPU: the NumPy statement of base-matrix AMP (tests/sc_ref.py) against the
oracle's uncoupled amp() where the two must agree, and on the coupled cases of
tests/sc_cases.py."""
import numpy as np
import pytest

from oracle import amp_oracle as orc
import sc_cases
import sc_ref


@pytest.mark.parametrize("wname", sorted(sc_cases.FLAT_W))
def test_statement_reduces_to_oracle_amp(wname):
    f = sc_cases.FLAT
    L, M, n, T = f["L"], f["M"], f["n"], f["T"]
    W = sc_cases.FLAT_W[wname]
    Pl = np.full(L, f["P"] / L)
    oAb, oAz, ordering = orc.sparc_transforms(L, M, n)
    idx, y = orc.rep_inputs(L, M, n, Pl, f["sigma"], oAb, f["seed"])
    ref, _ = orc._amp_core(y, Pl, L, M, T, oAb, oAz, None, early_stop=False)
    A = sc_ref.coupled_matrix(L, M, n, W, ordering)
    got, stop, phi, _ = sc_ref.amp_sc(y, Pl, W, L, M, T, A, early_stop=False)
    err = np.linalg.norm(got - ref.reshape(-1)) / np.linalg.norm(ref)
    print(f"W {wname}: statement vs oracle.amp norm-relative {err:.3e}")
    assert err <= 1e-12
    assert stop == T and np.all(phi > 0)


@pytest.mark.parametrize("omega,Lambda", [(1, 1), (2, 4), (3, 3), (3, 8), (4, 16)])
def test_base_matrix_columns_have_mean_one(omega, Lambda):
    from sparc_ldpc_amd import sc
    W = sc_ref.base_matrix(omega, Lambda)
    assert W.shape == (Lambda + omega - 1, Lambda)
    assert np.allclose(W.mean(axis=0), 1.0, rtol=1e-15, atol=0)
    assert (W >= 0).all() and (W.sum(axis=1) > 0).all()
    assert np.count_nonzero(W) == omega * Lambda
    assert np.array_equal(sc.base_matrix(omega, Lambda), W)  # the package's is the statement's


@pytest.mark.parametrize("case", sc_cases.LAYOUT_CASES, ids=lambda c: c.name)
def test_coupled_matrix_adjointness_and_column_norms(case):
    A = case.A
    rs = np.random.RandomState(7)
    beta, z = rs.randn(case.L * case.M), rs.randn(case.n)
    lhs, rhs = (A @ beta) @ z, beta @ (A.T @ z)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    # columns of mean 1 in W: every column of A has unit norm
    assert np.allclose((A ** 2).sum(axis=0), 1.0, rtol=1e-12)


@pytest.mark.parametrize("case,seed", sc_cases.DECODED, ids=lambda v: getattr(v, "name", str(v)))
def test_statement_decodes_every_section(case, seed):
    idx, y = case.rep(seed)
    beta, stop, phi, _ = sc_ref.amp_sc(y, case.Pl, case.W, case.L, case.M, 24, case.A)
    dec = orc.section_argmax(beta, case.L, case.M)
    print(f"case {case.name} seed {seed}: stop {stop}, correct {int((dec == idx).sum())}/{case.L}, "
          f"min phi {phi[:stop].min():.3g}")
    assert np.array_equal(dec, idx)
    assert stop == case.stops[seed]
    assert np.all(phi[stop:] == 0) and np.all(phi[:stop] > 0)
