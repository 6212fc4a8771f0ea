"""GPU: the spatially coupled decoder (sa_sc_*, kernels k_scsec / k_scrow,
sparc_ldpc_amd.sc) against the NumPy statement tests/sc_ref.py on the cases of
tests/sc_cases.py, in both precisions.  Tolerances: the project's own
(tests/test_gpu_parity.py), norm-relative."""
import ctypes as ct

import numpy as np
import pytest

from oracle import amp_oracle as orc
import sc_cases
import sc_ref
from test_sc_host import REFUSALS

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp64": 1e-11}
STOP64 = 3
PRECS = ("fp32", "fp64")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd as s
    return s


_OPS = {}


def transforms(sp, case, prec):
    """(Ab, Az) of a case's coupled design, one per (case shape, precision) and module."""
    key = (case.L, case.M, case.n, case.omega, case.Lambda, prec)
    if key not in _OPS:
        Ab, Az, ordering = sp.sc_transforms(case.L, case.M, case.n, case.W, precision=prec, device=0)
        assert np.array_equal(ordering, case.ordering)
        _OPS[key] = (Ab, Az)
    return _OPS[key]


_REF = {}


def reference(case, seed):
    """The statement's run of a rep, early stop off, T = 8: computed once, never changed."""
    key = (case.name, seed)
    if key not in _REF:
        idx, y = case.rep(seed)
        _, _, phi, snaps = sc_ref.amp_sc(y, case.Pl, case.W, case.L, case.M, 8, case.A, early_stop=False)
        for v in snaps.values():
            v.setflags(write=False)
        phi.setflags(write=False)
        _REF[key] = (idx, y, phi, snaps)
    return _REF[key]


# ---- 1. operators -------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", sc_cases.LAYOUT_CASES, ids=lambda c: c.name)
def test_operators(sp, case, prec):
    Ab, Az = transforms(sp, case, prec)
    rs = np.random.RandomState(11)
    beta, z = rs.randn(case.L * case.M, 1), rs.randn(case.n, 1)
    ab, az = Ab(beta), Az(z)
    assert ab.shape == (case.n, 1) and az.shape == (case.L * case.M, 1) and ab.dtype == az.dtype == np.float64
    e_ab, e_az = rel(ab, case.A @ beta), rel(az, case.A.T @ z)
    print(f"case {case.name} {prec}: Ab {e_ab:.2e} Az {e_az:.2e}")
    assert e_ab <= TOL[prec] and e_az <= TOL[prec]
    if prec == "fp64":
        lhs, rhs = (ab.T @ z).item(), (beta.T @ az).item()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    # a batch is its rows
    bb = rs.randn(3, case.L * case.M)
    out = Ab.op.Ab_batch(bb)
    for k in range(3):
        assert np.array_equal(out[k], Ab(bb[k]).reshape(-1))


# ---- 2. reduction to the shipped decoder -----------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("wname", sorted(sc_cases.FLAT_W))
def test_reduces_to_uncoupled_decoder(sp, wname, prec):
    f = sc_cases.FLAT
    L, M, n, T = f["L"], f["M"], f["n"], f["T"]
    W = sc_cases.FLAT_W[wname]
    Pl = np.full(L, f["P"] / L)
    oAb, oAz, _ = orc.sparc_transforms(L, M, n)
    idx, y = orc.rep_inputs(L, M, n, Pl, f["sigma"], oAb, f["seed"])
    ref = orc.amp(y, f["sigma"], Pl, L, M, T, oAb, oAz)
    Ab, Az, _ = sp.sc_transforms(L, M, n, W, precision=prec, device=0)
    got = sp.amp_sc(y, Pl, L, M, T, Ab, Az, early_stop=False)
    uAb, uAz, _ = sp.sparc_transforms(L, M, n, precision=prec, device=0)
    dev = sp.amp(y, f["sigma"], Pl, L, M, T, uAb, uAz, early_stop=False)
    assert got.shape == (L * M, 1)
    print(f"W {wname} {prec}: vs oracle.amp {rel(got, ref):.2e}, vs sp.amp {rel(got, dev):.2e}")
    assert rel(got, ref) <= TOL[prec]
    assert rel(got, dev) <= TOL[prec]
    dec = orc.section_argmax(got, L, M)
    assert np.array_equal(dec, orc.section_argmax(ref, L, M))
    assert np.array_equal(dec, orc.section_argmax(dev, L, M))


# ---- 3. trajectory ------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case,seed", sc_cases.TRAJ, ids=lambda v: getattr(v, "name", str(v)))
def test_trajectory(sp, case, seed, prec):
    Ab, Az = transforms(sp, case, prec)
    idx, y, phi_ref, snaps = reference(case, seed)
    for T in (1, 2, 4, 8):
        beta, iters, phi = sp.amp_sc_batch(y.reshape(1, -1), case.Pl, T, Ab, early_stop=False)
        assert beta.shape == (1, case.L * case.M) and phi.shape == (1, T, case.R) and iters[0] == T
        e_b = rel(beta, snaps[T])
        e_p = np.abs(phi[0] / phi_ref[:T] - 1).max()
        print(f"case {case.name} seed {seed} {prec} T={T}: beta {e_b:.2e} phi {e_p:.2e}")
        assert e_b <= TOL[prec], (T, e_b)
        assert e_p <= TOL[prec], (T, e_p)


# ---- 4. stop and decisions -------------------------------------------------------------
@pytest.mark.parametrize("case,seed", sc_cases.DECODED, ids=lambda v: getattr(v, "name", str(v)))
def test_stop_and_decisions(sp, case, seed):
    Ab, Az = transforms(sp, case, "fp64")
    idx, y = case.rep(seed)
    T = 24
    beta, iters, phi = sp.amp_sc_batch(y.reshape(1, -1), case.Pl, T, Ab)
    stop = int(iters[0])
    print(f"case {case.name} seed {seed}: stop {stop} (statement {case.stops[seed]})")
    assert abs(stop - case.stops[seed]) <= STOP64
    assert np.array_equal(orc.section_argmax(beta, case.L, case.M), idx)
    assert stop < T and np.all(phi[0, stop:] == 0) and np.all(phi[0, :stop] > 0)
    # the single-codeword form returns the same estimate
    assert np.array_equal(sp.amp_sc(y, case.Pl, case.L, case.M, T, Ab, Az).reshape(-1), beta[0])


# ---- 5. batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("early_stop", [False, True], ids=["nostop", "stop"])
@pytest.mark.parametrize("prec", PRECS)
def test_batch_is_its_codewords_bit_for_bit(sp, prec, early_stop):
    case = sc_cases.D
    Ab, Az = transforms(sp, case, prec)
    ys = np.stack([case.rep(s)[1] for s in case.seeds])
    T = 12
    beta, iters, phi = sp.amp_sc_batch(ys, case.Pl, T, Ab, early_stop=early_stop)
    beta2, iters2, phi2 = sp.amp_sc_batch(ys, case.Pl, T, Ab, early_stop=early_stop)
    assert np.array_equal(beta, beta2) and np.array_equal(iters, iters2) and np.array_equal(phi, phi2)
    for k in range(3):
        b1, i1, p1 = sp.amp_sc_batch(ys[k:k + 1], case.Pl, T, Ab, early_stop=early_stop)
        assert np.array_equal(b1[0], beta[k]) and i1[0] == iters[k] and np.array_equal(p1[0], phi[k])


# ---- 6. Monte Carlo ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_mc_decode_equals_batch_decode_of_the_same_draws(sp, prec):
    from sparc_ldpc_amd.harness import _draw_reps
    case = sc_cases.B
    Ab, Az = transforms(sp, case, prec)
    seeds = list(range(16))
    T = 24
    errs, its, dec = sp.mc_decode_sc(Ab, case.Pl, case.sigma, T, seeds, batch=5)
    idx, noise = _draw_reps(seeds, case.L, case.M, case.n, case.sigma)
    beta0 = np.zeros((16, case.L * case.M))
    cl = np.sqrt(case.n * case.Pl)
    for k in range(16):
        beta0[k, np.arange(case.L) * case.M + idx[k]] = cl
    y = Ab.op.Ab_batch(beta0) + noise
    beta, iters, _ = sp.amp_sc_batch(y, case.Pl, T, Ab)
    want = beta.reshape(16, case.L, case.M).argmax(axis=2)
    werr = np.array([sum(bin(int(v)).count("1") for v in (want[k] ^ idx[k])) for k in range(16)])
    assert dec.dtype == its.dtype == errs.dtype == np.int32
    assert np.array_equal(dec, want)
    assert np.array_equal(its, iters)
    assert np.array_equal(errs, werr)


# ---- 7. refusals through the ABI ----------------------------------------------------------
def _create(sp, lib, parent, W):
    W = np.ascontiguousarray(W, dtype=np.float64)
    out = ct.c_void_p(0xdead)
    rc = lib.sa_sc_create(parent.ctx, W.shape[0], W.shape[1], W.ctypes.data_as(ct.POINTER(ct.c_double)), ct.byref(out))
    return rc, out.value, lib.sa_last_error().decode()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_through_the_abi(sp, lib_gpu, name):
    L, M, n, W, status, text = REFUSALS[name]
    parent = sp.SparcOperator(L, M, n, orc.make_ordering(L, M, n, 0), "hadamard", "fp32", 0)
    rc, out, msg = _create(sp, lib_gpu, parent, W)
    assert rc == status, (rc, msg)
    assert text in msg
    assert out == 0xdead  # nothing written


def test_dense_parent_is_unsupported(sp, lib_gpu):
    A = sc_cases.A
    parent = sp.SparcOperator(A.L, A.M, A.n, A.ordering, "dense", "fp32", 0)
    rc, out, msg = _create(sp, lib_gpu, parent, A.W)
    assert rc == sp._lib.SA_ERR_UNSUPPORTED and "Hadamard" in msg and out == 0xdead
    with pytest.raises(sp.SparcAmpError):
        sp.sc.CoupledOperator(parent, A.W)


def test_bad_call_arguments_leave_outputs_untouched(sp, lib_gpu):
    case = sc_cases.C
    Ab, Az = transforms(sp, case, "fp32")
    sc = Ab.op._sc
    D = ct.POINTER(ct.c_double)
    out = np.full(case.n, 7.0)
    beta = np.zeros(case.L * case.M)
    assert lib_gpu.sa_sc_Ab(sc, 0, beta.ctypes.data_as(D), out.ctypes.data_as(D)) == sp._lib.SA_ERR_ARG
    assert lib_gpu.sa_sc_Ab(None, 1, beta.ctypes.data_as(D), out.ctypes.data_as(D)) == sp._lib.SA_ERR_ARG
    bout = np.full(case.L * case.M, 7.0)
    Pl = case.Pl.copy()
    Pl[3] = -1.0
    y = np.zeros(case.n)
    rc = lib_gpu.sa_sc_amp(sc, 1, y.ctypes.data_as(D), Pl.ctypes.data_as(D), 4, bout.ctypes.data_as(D), None, None, 0)
    assert rc == sp._lib.SA_ERR_ARG and b"Pl" in lib_gpu.sa_last_error()
    rc = lib_gpu.sa_sc_amp(sc, 1, y.ctypes.data_as(D), case.Pl.ctypes.data_as(D), 4, bout.ctypes.data_as(D), None, None, 64)
    assert rc == sp._lib.SA_ERR_ARG and b"flags" in lib_gpu.sa_last_error()
    assert (out == 7.0).all() and (bout == 7.0).all()
