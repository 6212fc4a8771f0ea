"""CPU: oracle/glue_oracle.py (the long double restatement of the SPARC <-> LDPC
glue that tests/test_gpu_glue.py holds the device kernels to) against fixtures
captured from the reference (tests/golden/ldpc.npz) and against the FWHT
oracle's Ab.  Bars of test_joint_host.test_host_sp2bp_bp2sp_helpers: p exact
in binary64, sp within 1e-13."""
import numpy as np

from conftest import golden
from oracle import amp_oracle as orc
from oracle import glue_oracle as go
from oracle import ldpc_oracle as lo

CASES = ((6, 8), (4, 64), (3, 512))
F64_MAX = np.finfo(np.float64).max


def test_long_double_is_wider_than_binary64():
    """The device tests' bounds are a few binary64 ulp: the oracle must not
    spend them itself."""
    assert np.finfo(go.LD).eps <= 2.0 ** -63


def test_sp2bp_and_llr_match_reference_fixtures():
    g = golden("ldpc.npz")
    for L, M in CASES:
        beta, p_ref, llr_ref = (g[f"sp2bp|{L}|{M}|{k}"] for k in ("beta", "p", "llr"))
        p = go.sp2bp(beta, L, M)
        assert p.dtype == np.float64 and np.array_equal(p, p_ref)
        # the long double accumulator gives the same sums to binary64 rounding of each of the M/2 additions
        pl = go.sp2bp(beta.astype(go.LD), L, M)
        assert pl.dtype == go.LD
        assert np.all(np.abs(pl - p_ref) <= (M // 2) * 2.0 ** -53 * np.abs(p_ref))
        # LLRs through llr_of_p, and through llr() with c_l = 1 (n Pl_l = 1)
        for got in (go.llr_of_p(p), go.llr(beta[None, :], 1, np.ones(L), L, M, 0, L)[0][0]):
            got = np.asarray(got, dtype=np.float64)
            sat = np.abs(llr_ref) == F64_MAX
            assert sat.any() and np.array_equal(got[sat], llr_ref[sat])  # the decided section of the fixture
            assert np.array_equal(got == 0.0, llr_ref == 0.0)
            with np.errstate(divide="ignore"):
                cond = np.abs(np.log(p_ref)) + np.abs(np.log1p(-p_ref))
            # the reference's two binary64 logs and their difference: 1 ulp each of its terms
            assert np.all(np.abs(got - llr_ref)[~sat] <= 4 * 2.0 ** -53 * cond[~sat])


def test_llr_section_range_and_power():
    """llr() divides section l by its own c_l and returns sections [l0, l0 + ns)."""
    L, M, n, l0, ns = 5, 8, 24, 2, 2
    rs = np.random.RandomState(3)
    Pl = 2.0 ** (-np.arange(L) / L)
    w = rs.dirichlet(np.ones(M), (2, L))
    beta = (w * np.sqrt(n * Pl)[None, :, None]).reshape(2, L * M)
    got, p = go.llr(beta, n, Pl, L, M, l0, ns)
    want = np.stack([[w[b, l, [m for m in range(M) if (m >> (2 - t)) & 1]].sum()
                      for l in range(l0, l0 + ns) for t in range(3)] for b in range(2)])
    np.testing.assert_allclose(p, want, rtol=1e-14)
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), np.log(1 - want) - np.log(want), rtol=1e-12)


def test_llr_of_p_edges():
    got = go.llr_of_p(np.array([0.0, 1.0, 1.0 + 2.0 ** -52, 0.5, np.nan]))
    assert np.array_equal(np.asarray(got, dtype=np.float64), [F64_MAX, -F64_MAX, 0.0, 0.0, 0.0])


def test_bp2sp_matches_reference_fixtures():
    g = golden("ldpc.npz")
    for L, M in CASES:
        if f"bp2sp|{L}|{M}|v" not in g:
            continue
        sp = go.bp2sp(g[f"bp2sp|{L}|{M}|v"], L, M)
        np.testing.assert_allclose(np.asarray(sp, dtype=np.float64), g[f"bp2sp|{L}|{M}|sp"], rtol=1e-13, atol=0)
        np.testing.assert_allclose(np.asarray(sp.reshape(L, M).sum(axis=1), dtype=np.float64), 1.0, rtol=1e-15)


def test_soft_beta0_rescale_hard_and_threshold():
    L, M, n, l0, ns, lgm = 4, 8, 20, 1, 2, 3
    rs = np.random.RandomState(5)
    Pl = 2.0 ** (-np.arange(L) / L)
    c = np.sqrt(n * Pl)
    beta = rs.rand(2, L * M) + 0.1
    app = rs.randn(2, ns * lgm) * 2
    out = np.asarray(go.soft_beta0(beta, app, n, Pl, L, M, l0, ns), dtype=np.float64).reshape(2, L, M)
    keep = [l for l in range(L) if not l0 <= l < l0 + ns]
    np.testing.assert_allclose(out[:, keep], beta.reshape(2, L, M)[:, keep], rtol=1e-15)
    bp = 1 / (1 + np.exp(app))
    for b in range(2):  # the reference's own bp2sp restatement (ldpc_oracle.bp2sp) on the same marginals
        np.testing.assert_allclose(out[b, l0:l0 + ns].reshape(-1),
                                   lo.bp2sp(bp[b], ns, M) * np.repeat(c[l0:l0 + ns], M), rtol=1e-13)
    # hard indices: app < 0, MSB first; NaN, 0.0 and -0.0 are not negative
    h = go.hard_indices(np.array([[-1.0, 2.0, -np.inf, 0.0, -0.0, np.nan, -F64_MAX, F64_MAX, -1e-300]]), M)
    assert np.array_equal(h, [[0b101, 0b000, 0b101]])
    # threshold: decided iff exactly one entry above
    big = np.array([[-9.0, 9.0, -9.0, 0.0, 9.0, 9.0, np.nan, 1.0, 1.0]])  # 101 decided; 0xx split in two halves; NaN
    idx, sp = go.threshold_indices(big, 3, M, 0.3)
    assert np.array_equal(idx, [[0b101, -1, -1]])
    assert np.array_equal((np.asarray(sp[0, 1], dtype=np.float64) > 0.3).nonzero()[0], [0, 4])
    idx7, _ = go.threshold_indices(big, 3, M, 0.7)
    assert np.array_equal(idx7, [[0b101, -1, -1]])  # nothing of section 1 passes 0.7: still undecided


def test_encode_and_cancel_against_fwht_oracle():
    """encode = Ab of the one-hot β (rtol 1e-12, the FWHT oracle's binary64
    butterflies), at a non-flat allocation, n not a multiple of anything and
    w > 2 M; cancel undoes encode on the decided sections only."""
    for L, M, n in ((10, 16, 300), (5, 128, 70), (12, 2, 20)):
        Ab, _, ordering = orc.sparc_transforms(L, M, n)
        Pl = 2.0 ** (-np.arange(L) / L)
        Pl *= 2.0 / Pl.sum()
        rs = np.random.RandomState(L)
        idx = rs.randint(0, M, (2, L))
        idx[0, 0], idx[0, 1] = 0, M - 1
        beta = np.asarray(go.onehot(n, Pl, M, idx), dtype=np.float64)
        assert np.array_equal(beta.reshape(2, L, M).argmax(axis=2), idx)
        assert np.array_equal(np.sort(beta.reshape(2, L, M), axis=2)[:, :, -1], np.tile(np.sqrt(n * Pl), (2, 1)))
        assert np.count_nonzero(beta) == 2 * L
        y = go.encode(ordering, M, n, Pl, idx)
        for b in range(2):
            want = Ab(beta[b]).reshape(-1)
            np.testing.assert_allclose(np.asarray(y[b], dtype=np.float64), want, rtol=1e-12, atol=0)
        # the dense matrix's definition, column by column
        A = orc.dense_design_matrix(L, M, n, ordering)
        np.testing.assert_allclose(np.asarray(y, dtype=np.float64), beta @ A.T, rtol=1e-12, atol=1e-13)
        # cancel: scaled, with kept (-1) sections, over a sub-range
        noise = rs.randn(2, n)
        part = idx.copy()
        part[0, ::3] = -1
        part[1, :] = -1
        got = go.cancel(ordering, M, n, Pl, noise, part, scale=0.37)
        kept = np.asarray(go.onehot(n, Pl, M, part, 0.37), dtype=np.float64)
        np.testing.assert_allclose(np.asarray(got, dtype=np.float64), noise - kept @ A.T, rtol=1e-12, atol=1e-13)
        assert np.array_equal(got[1], noise[1].astype(go.LD))  # nothing decided: y unchanged, exactly
        l0, ns = L // 3, L // 2
        sub = go.cancel(ordering, M, n, Pl, noise, idx[:, l0:l0 + ns], sections=np.arange(l0, l0 + ns))
        only = np.full_like(idx, -1)
        only[:, l0:l0 + ns] = idx[:, l0:l0 + ns]
        np.testing.assert_array_equal(sub, go.cancel(ordering, M, n, Pl, noise, only))
