"""CPU: the NumPy statement of the coupled beta_0 start and of the joint coupled
decoder (tests/sc_joint_ref.py) against the statements and oracles it must
agree with: sc_ref.amp_sc and sc_wave_ref.amp_sc_wave bit for bit without a
beta_0, the oracle's uncoupled beta_0 loop at W = [[1]], and the reference's own
soft / hard joint reps (tests/golden/joint.npz) at W = [[1]]."""
import numpy as np
import pytest

from conftest import golden
from oracle import amp_oracle as orc
from oracle import glue_oracle as go
import sc_cases
import sc_joint_cases as jc
import sc_joint_ref as ref
import sc_ref
import sc_wave_cases as wc
import sc_wave_ref


@pytest.mark.parametrize("case,seed", sc_cases.TRAJ, ids=lambda v: getattr(v, "name", str(v)))
def test_without_a_start_it_is_the_coupled_statement_bit_for_bit(case, seed):
    _, y = case.rep(seed)
    for es in (True, False):
        T = 24 if es else 8
        b0, s0, p0, snaps0 = sc_ref.amp_sc(y, case.Pl, case.W, case.L, case.M, T, case.A, early_stop=es)
        for start in (None, np.zeros(case.L * case.M)):
            b1, s1, p1, live, snaps1, _ = ref.amp_sc_start(y, case.Pl, case.W, case.L, case.M, T, case.A, beta0=start,
                                                           early_stop=es)
            assert np.array_equal(b0, b1) and s0 == s1 and np.array_equal(p0, p1)
            assert all(np.array_equal(snaps0[t], snaps1[t]) for t in snaps0)
            assert np.array_equal(live[:s1], np.ones((s1, case.C), dtype=np.uint8)) and not live[s1:].any()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("w,seed", wc.TABLE, ids=lambda v: getattr(v, "name", str(v)))
def test_with_tolerances_it_is_the_wave_statement_bit_for_bit(w, seed, dt):
    c = w.case
    _, y = c.rep(seed)
    a = sc_wave_ref.amp_sc_wave(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, w.stop_tol, w.freeze_tol, dtype=dt)
    for start in (None, np.zeros(c.L * c.M)):
        b = ref.amp_sc_start(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, beta0=start, stop_tol=w.stop_tol, freeze_tol=w.freeze_tol,
                             dtype=dt)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert a[5] == b[5] and b[0].dtype == dt


def test_at_the_flat_base_matrix_a_start_is_the_oracles_start():
    f = sc_cases.FLAT
    L, M, n, T = f["L"], f["M"], f["n"], f["T"]
    Pl = np.full(L, f["P"] / L)
    oAb, oAz, ordering = orc.sparc_transforms(L, M, n)
    idx, y = orc.rep_inputs(L, M, n, Pl, f["sigma"], oAb, f["seed"])
    rs = np.random.RandomState(5)
    lgm = int(np.log2(M))
    soft = np.asarray(go.soft_beta0(np.zeros((1, L * M)), rs.randn(1, L * lgm) * 3, n, Pl, L, M, 0, L), dtype=np.float64)[0]
    wrong = np.zeros(L * M)
    moved = np.where(np.arange(L) % 5 == 0, (idx + 1) % M, idx)
    wrong[np.arange(L) * M + moved] = np.sqrt(n * Pl)
    A = sc_ref.coupled_matrix(L, M, n, np.ones((1, 1)), ordering)
    W1 = np.ones((1, 1))
    for name, b0 in (("soft", soft), ("wrong", wrong)):
        for Tk in (1, 2, T):
            want, _ = orc._amp_core(y, Pl, L, M, Tk, oAb, oAz, b0, early_stop=False)
            got = ref.amp_sc_start(y, Pl, W1, L, M, Tk, A, beta0=b0, early_stop=False)[0]
            err = np.linalg.norm(got - want.reshape(-1)) / np.linalg.norm(want)
            print(f"start {name} T={Tk}: statement vs oracle.amp norm-relative {err:.3e}")
            assert err <= 1e-12  # tests/test_sc_ref.py's bar for the zero start
        # the start is read: one iteration from it is not one iteration from zero
        assert not np.array_equal(ref.amp_sc_start(y, Pl, W1, L, M, 1, A, early_stop=False)[0],
                                  ref.amp_sc_start(y, Pl, W1, L, M, 1, A, beta0=b0, early_stop=False)[0])


# ---- the reference's own joint reps at W = [[1]] -------------------------------------------
def _golden_keys():
    g = golden("joint.npz")
    return sorted({k.rsplit("|", 1)[0] for k in g if k.count("|") == 3 and k.split("|")[0] in ("small", "mid", "noisy")
                   and k.split("|")[1] in ("soft", "hard")})


_FLAT = {}


def _flat_case(L, M, n, P, sigma):
    key = (L, M, n)
    if key not in _FLAT:
        _FLAT[key] = sc_cases.Case("G", L, M, n, 1, 1, P, sigma, ())
    c = _FLAT[key]
    assert c.P == P
    return c


@pytest.mark.parametrize("key", _golden_keys())
def test_joint_rep_reproduces_the_reference_at_the_flat_base_matrix(key):
    G = golden("joint.npz")
    tag, mode, seed = key.split("|")
    L, M, P, r, T, z, sigma = G[f"{tag}|cfg"]
    L, M, T, z = int(L), int(M), int(T), int(z)
    n = int(L * np.log2(M) / r)
    assert (L, M, n, z) == (64, 16, 256, 8)
    case = _flat_case(L, M, n, float(P), float(sigma))
    np.random.seed(int(seed))  # the seeded global stream, as tests/test_gpu_joint.py draws its reps
    rep = ref.joint_rep(case, jc.graph(), None, mode, 2, T, rs=np.random, sigma=float(sigma))
    assert np.array_equal(rep["idx"], G[key + "|idx"])
    tb = L * int(np.log2(M))
    got = np.array([e / tb for e in rep["amp"]] + [e / tb for e in rep["ldpc"]])
    want = G[key + "|ber"]
    its = [int(G[key + f"|it{k}"][0]) for k in range(4) if key + f"|it{k}" in G]
    print(f"{key}: BER {got} reference {want}; BP iterations {rep['bp_iters']} reference {its}")
    assert got[0] == want[0]
    if all(i < 200 for i in its):
        assert rep["bp_iters"] == its
        np.testing.assert_array_equal(got, want)
    else:
        assert np.max(np.abs(got - want)) <= 0.03
