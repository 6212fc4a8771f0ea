"""GPU: coupled state evolution on the device (sa_sc_se, csrc/sa_se.hip;
sparc_ldpc_amd.sc_state_evolution / sc_search / CoupledOperator.state_evolution)
against its NumPy statement (tests/sc_se_ref.py) on the cases of
tests/sc_se_cases.py.

Tolerance: per case, 64 x the largest gap between the statement in binary64
and in np.longdouble (recorded by scripts/sc_se_case_seeds.py from the
statement alone), absolute, for phi, tau2, x and sections, as
tests/test_gpu_se.py has it.  The miss counts per block and the predicted stop
indices must be equal: every case's seed was chosen so that each miss
comparison has a relative margin of at least 1e-9 and the two precisions of
the statement agree on the stop index.  Everything the device is compared with
itself on is compared by equality."""
import ctypes as ct

import numpy as np
import pytest

import sc_cases
import sc_se_cases as scc
import se_cases

pytestmark = pytest.mark.gpu

NAMES = list(scc.CASES)
FIELDS = ("phi", "tau2", "x", "miss", "ser")


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_RUNS = {}


def _call(sp, c, **kw):
    kw.setdefault("draws", c.U)
    return sp.sc_state_evolution(c.Pl, c.M, c.n, c.W, c.sigma, c.T, **kw)


def _host_rows_run(sp, name):
    """The device's result on the case's NumPy rows, computed once."""
    if name not in _RUNS:
        _RUNS[name] = _call(sp, scc.case(name))
    return _RUNS[name]


def _same_bits(a, b):
    for f in FIELDS:
        for va, vb in zip(getattr(a, f), getattr(b, f)):
            np.testing.assert_array_equal(va, vb, err_msg=f)
    for f in ("ser_all", "stop", "sections"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


@pytest.mark.parametrize("name", NAMES)
def test_against_the_statement(sp, name):
    c = scc.case(name)
    assert c.margin >= scc.MARGIN
    r = _host_rows_run(sp, name)
    assert r.sections.shape == (c.B, c.L) and r.ser_all.shape == (c.B, c.T) and r.ms > 0
    for b in range(c.B):
        R, C = c.R[b], c.C[b]
        assert r.phi[b].shape == (c.T + 1, R) and r.tau2[b].shape == (c.T, C) and r.x[b].shape == (c.T, C)
        assert r.miss[b].shape == (c.T, C) and r.miss[b].dtype == np.int64
        d = [float(np.max(np.abs(got - want))) for got, want in
             ((r.phi[b], c.phi[b]), (r.tau2[b], c.tau2[b]), (r.x[b], c.x[b]), (r.sections[b], c.E[b]))]
        print(f"{name}[{b}]: tol {c.tol:.3e}; phi {d[0]:.3e}, tau2 {d[1]:.3e}, x {d[2]:.3e}, sections {d[3]:.3e}; "
              f"stop {int(r.stop[b])} (statement {c.stop[b]}); misses {r.miss[b][-1].tolist()}; {r.ms:.3f} ms")
        np.testing.assert_array_equal(r.miss[b], c.miss[b])
        assert int(r.stop[b]) == c.stop[b]
        assert max(d) <= c.tol
        np.testing.assert_array_equal(r.phi[b][0], c.phi[b][0])  # sigma^2 + W P_c: the same operations
        np.testing.assert_array_equal(r.ser[b], c.miss[b] / float((c.L // C) * c.S))
        np.testing.assert_array_equal(r.ser_all[b], c.miss[b].sum(axis=1) / float(c.L * c.S))


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_same_bits(sp, name):
    _same_bits(_host_rows_run(sp, name), _call(sp, scc.case(name)))


@pytest.mark.parametrize("name", NAMES)
def test_seeded_path_is_the_U_path(sp, name):
    c = scc.case(name)
    Ud = sp.se_draws(c.seeds, c.M)
    seeded = _call(sp, c, draws="device", samples=c.S, seed=c.seed)
    _same_bits(seeded, _call(sp, c, draws=Ud))


@pytest.mark.parametrize("name", NAMES)
def test_skip_is_no_skip(sp, name):
    _same_bits(_host_rows_run(sp, name), _call(sp, scc.case(name), skip=False))


def test_batch_is_its_configurations_alone(sp):
    c = scc.case("batch_mixed")
    r = _host_rows_run(sp, "batch_mixed")
    assert c.B == 3
    for b in range(c.B):
        one = sp.sc_state_evolution(c.Pl[b], c.M, c.n[b], c.W[b], c.sigma[b], c.T, draws=c.U)
        assert one.phi.shape == (c.T + 1, c.R[b]) and isinstance(one.stop, int)
        rb = r.config(b)
        for f in FIELDS + ("ser_all", "sections"):
            np.testing.assert_array_equal(getattr(one, f), getattr(rb, f), err_msg=f"{f}, configuration {b}")
        assert one.stop == rb.stop


def test_sc_search_is_its_single_calls(sp):
    L, M, n, P, sigma, T, S = 24, 32, 100, 2.0, 0.6, 12, 17
    omegas, Lambdas = [1, 2, 3], [2, 4]
    res = sp.sc_search(L, M, n, P, sigma, omegas, Lambdas, T, samples=S, seed=2)
    shape = (3, 2)
    assert res.n.shape == shape and res.ser.shape == shape and res.stop.shape == shape and res.iters.shape == shape
    keys = []
    for i, om in enumerate(omegas):
        for j, lam in enumerate(Lambdas):
            R = lam + om - 1
            n_used = R * -(-n // R)
            assert res.n[i, j] == n_used and n <= n_used < n + R
            assert res.rate[i, j] == L * np.log2(M) / n_used <= L * np.log2(M) / n
            one = sp.sc_state_evolution(np.full(L, P / L), M, n_used, sp.base_matrix(om, lam), sigma, T, samples=S, seed=2)
            rb = res.result.config(i * len(Lambdas) + j)
            for f in FIELDS + ("ser_all", "sections"):
                np.testing.assert_array_equal(getattr(one, f), getattr(rb, f), err_msg=f"{f}, ({om}, {lam})")
            assert res.ser[i, j] == one.ser_all[-1] and res.stop[i, j] == one.stop == rb.stop
            first = int(np.argmax(one.ser_all == one.ser_all[-1])) + 1
            assert res.iters[i, j] == first and 1 <= first <= T
            keys.append((one.ser_all[-1], one.stop, i * len(Lambdas) + j, (om, lam)))
    assert res.best == min(keys)[3]
    # a pair that cannot run is named, never dropped
    with pytest.raises(ValueError, match=r"\(2, 5\)"):
        sp.sc_search(L, M, n, P, sigma, [2], [4, 5], T, samples=S)
    with pytest.raises(ValueError, match=r"\(42, 24\)"):
        sp.sc_search(L, M, n, P, sigma, [2, 42], [24], T, samples=S)


# ---- padding and tail rows ----------------------------------------------------------

_SENTINEL = -77.25


def _raw(lib, L, M, configs, T, S, seeds=None, U=None, Rmax=None, Cmax=None, flags=0, B=None):
    """sa_sc_se called as C would, on outputs filled with a sentinel.
    configs: [(n, W, sigma, Pl)]."""
    from sparc_ldpc_amd import _lib
    nb = len(configs) if B is None else B
    Ws = [np.asarray(c[1], dtype=np.float64) for c in configs]
    ns = np.array([c[0] for c in configs], dtype=np.int32)
    Rs = np.array([w.shape[0] for w in Ws], dtype=np.int32)
    Cs = np.array([w.shape[1] for w in Ws], dtype=np.int32)
    Wcat = np.ascontiguousarray(np.concatenate([w.reshape(-1) for w in Ws]))
    sig = np.array([c[2] for c in configs], dtype=np.float64)
    Pl = np.ascontiguousarray(np.array([c[3] for c in configs], dtype=np.float64))
    Rmax = int(Rs.max()) if Rmax is None else Rmax
    Cmax = int(Cs.max()) if Cmax is None else Cmax
    mb, mt, mr, mc = max(nb, 1), max(T, 1), max(Rmax, int(Rs.max())), max(Cmax, int(Cs.max()))
    outs = [np.full((mb, mt + 1, mr), _SENTINEL), np.full((mb, mt, mc), _SENTINEL), np.full((mb, mt, mc), _SENTINEL),
            np.full((mb, mt, mc), -77, dtype=np.int64), np.full(mb, -77, dtype=np.int32), np.full((mb, max(L, 1)), _SENTINEL)]
    ms = ct.c_double(_SENTINEL)
    seeds = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
    U = None if U is None else np.ascontiguousarray(U, dtype=np.float64)
    ip = ct.POINTER(ct.c_int)
    rc = lib.sa_sc_se(0, nb, L, M, ns.ctypes.data_as(ip), Rs.ctypes.data_as(ip), Cs.ctypes.data_as(ip), _lib.dptr(Wcat),
                      _lib.dptr(Pl), _lib.dptr(sig), T, S,
                      None if seeds is None else seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)),
                      None if U is None else _lib.dptr(U), Rmax, Cmax, flags, _lib.dptr(outs[0]), _lib.dptr(outs[1]),
                      _lib.dptr(outs[2]), outs[3].ctypes.data_as(ct.POINTER(ct.c_int64)), outs[4].ctypes.data_as(ip),
                      _lib.dptr(outs[5]), ct.cast(ct.pointer(ms), ct.POINTER(ct.c_double)))
    untouched = (all(np.all(o == _SENTINEL) for o in (outs[0], outs[1], outs[2], outs[5])) and np.all(outs[3] == -77)
                 and np.all(outs[4] == -77) and ms.value == _SENTINEL)
    return rc, lib.sa_last_error().decode(), untouched, outs


def test_padding_is_zero(sp, lib_gpu):
    from sparc_ldpc_amd import _lib
    c = scc.case("batch_mixed")
    configs = [(c.n[b], c.W[b], c.sigma[b], c.Pl[b]) for b in range(c.B)]
    Rmax, Cmax = max(c.R) + 2, max(c.C) + 1  # wider than any configuration
    rc, msg, untouched, (phi, tau2, x, miss, stop, sec) = _raw(lib_gpu, c.L, c.M, configs, c.T, c.S, U=c.U, Rmax=Rmax, Cmax=Cmax)
    assert rc == _lib.SA_OK and not untouched, msg
    r = _host_rows_run(sp, "batch_mixed")
    for b in range(c.B):
        R, C = c.R[b], c.C[b]
        assert np.all(phi[b, :, R:] == 0) and np.all(tau2[b, :, C:] == 0) and np.all(x[b, :, C:] == 0)
        assert np.all(miss[b, :, C:] == 0)
        np.testing.assert_array_equal(phi[b, :, :R], r.phi[b])
        np.testing.assert_array_equal(tau2[b, :, :C], r.tau2[b])
        np.testing.assert_array_equal(x[b, :, :C], r.x[b])
        np.testing.assert_array_equal(miss[b, :, :C], r.miss[b])
        assert np.all(phi[b, :, :R] > 0) and np.all(tau2[b, :, :C] > 0)
    np.testing.assert_array_equal(stop, r.stop)
    np.testing.assert_array_equal(sec, r.sections)


def test_rows_from_the_stop_index_on_are_the_stop_row(sp):
    c = scc.case("band_2_4")
    r = _host_rows_run(sp, "band_2_4")
    stop = int(r.stop[0])
    assert 1 <= stop < c.T - 8
    np.testing.assert_array_equal(r.phi[0][stop], r.phi[0][stop - 1])
    for t in range(stop, c.T + 1):
        np.testing.assert_array_equal(r.phi[0][t], r.phi[0][stop], err_msg=f"row {t}")
    for t in range(stop, c.T):
        np.testing.assert_array_equal(r.tau2[0][t], r.tau2[0][stop - 1])
        np.testing.assert_array_equal(r.x[0][t], r.x[0][stop - 1])
        np.testing.assert_array_equal(r.miss[0][t], r.miss[0][stop - 1])
    assert not np.array_equal(r.phi[0][stop - 1], r.phi[0][stop - 2]) or stop == 1


# ---- against the uncoupled path and the decoder's layout ----------------------------------

@pytest.mark.parametrize("name", ["flat_1x1", "batch_mixed"])
def test_flat_base_matrix_is_state_evolution(sp, name):
    c = scc.case(name)
    assert c.W[0].shape == (1, 1) and c.W[0][0, 0] == 1
    r = _host_rows_run(sp, name).config(0)
    f = sp.state_evolution(c.Pl[0], c.M, c.n[0], c.sigma[0], c.T, draws=c.U)
    d = [float(np.max(np.abs(r.phi[:, 0] - f.tau2))), float(np.max(np.abs(r.tau2[:, 0] - f.tau2[:c.T]))),
         float(np.max(np.abs(r.x[:, 0] - f.x))), float(np.max(np.abs(r.sections - f.sections)))]
    print(f"{name}: tol {c.tol:.3e}; phi {d[0]:.3e}, tau2 {d[1]:.3e}, x {d[2]:.3e}, sections {d[3]:.3e}")
    assert max(d) <= c.tol
    np.testing.assert_array_equal(r.miss[:, 0], f.miss)
    np.testing.assert_array_equal(r.ser_all, f.ser)


def test_operator_state_evolution(sp):
    A = sc_cases.A
    T, S = 6, 9
    Ab, Az, _ = sp.sc_transforms(A.L, A.M, A.n, A.W, device=0)
    op = Ab.op
    r = op.state_evolution(A.Pl, A.sigma, T, samples=S, seed=4)
    same = sp.sc_state_evolution(A.Pl, A.M, A.n, A.W, A.sigma, T, samples=S, seed=4)
    for f in FIELDS + ("ser_all", "sections"):
        np.testing.assert_array_equal(getattr(r, f), getattr(same, f), err_msg=f)
    assert r.stop == same.stop
    assert r.phi.shape == (T + 1, op.R) and r.tau2.shape == (T, op.C) and r.sections.shape == (op.L,)
    # phi^0 = sigma^2 + W P_c: what the first row of the decoder's trace estimates
    Pc = [0.0] * A.C
    for l in range(A.L):
        Pc[l // (A.L // A.C)] += A.Pl[l]
    for row in range(A.R):
        acc = 0.0
        for k in range(A.C):
            acc += A.W[row, k] * Pc[k]
        assert r.phi[0, row] == A.sigma * A.sigma + acc
    idx, y = A.rep(A.seeds[0])
    _, _, trace = sp.amp_sc_batch(y.reshape(1, -1), A.Pl, T, Ab, early_stop=False)
    assert trace.shape == (1, T, op.R) and r.phi[:T].shape == trace.shape[1:]


# ---- refusals -------------------------------------------------------------------------

def test_refusals(sp, lib_gpu):
    from sparc_ldpc_amd import _lib
    c = scc.case("band_2_4")
    L, M, T, S = c.L, c.M, 3, 5
    n, W, sg, Pl = c.n[0], c.W[0], c.sigma[0], c.Pl[0]
    U = np.random.RandomState(1).randn(S, M)
    seeds = np.arange(S)
    rc, msg, untouched, _ = _raw(lib_gpu, L, M, [(n, W, sg, Pl)], T, S, U=U)
    assert rc == _lib.SA_OK and not untouched, msg

    def w_with(at, v):
        w = W.copy()
        w[at] = v
        return w

    def pl_with(sl, v):
        p = Pl.copy()
        p[sl] = v
        return p

    big = _lib.SA_SC_MAX_BLOCKS + 1
    ARG, UNS = _lib.SA_ERR_ARG, _lib.SA_ERR_UNSUPPORTED
    bad = [  # (status, what the message must name, arguments)
        (ARG, "does not divide n", dict(configs=[(161, W, sg, Pl)])),
        (ARG, "does not divide L", dict(L=30, configs=[(n, W, sg, Pl[:30])])),
        (ARG, "W[1,0] is negative", dict(configs=[(n, w_with((1, 0), -0.5), sg, Pl)])),
        (ARG, "W[2,1] is not finite", dict(configs=[(n, w_with((2, 1), np.nan), sg, Pl)])),
        (ARG, "W[2,2] is not finite", dict(configs=[(n, w_with((2, 2), np.inf), sg, Pl)])),
        (ARG, "W row 4", dict(configs=[(n, w_with((4, slice(None)), 0.0), sg, Pl)])),
        (ARG, "W column 1", dict(configs=[(n, w_with((slice(None), 1), 0.0), sg, Pl)])),
        (UNS, "R above SA_SC_MAX_BLOCKS", dict(L=4, configs=[(2 * big, np.ones((big, 1)), sg, np.ones(4))])),
        (UNS, "C above SA_SC_MAX_BLOCKS", dict(L=big, configs=[(128, np.ones((1, big)), sg, np.ones(big))])),
        (ARG, "M < 2", dict(M=1, U=U[:, :1])),
        (UNS, "SA_SE_MAX_M", dict(M=scc.MAX_M + 1, U=np.zeros((S, scc.MAX_M + 1)))),
        (ARG, "sigma", dict(configs=[(n, W, 0.0, Pl)])), (ARG, "sigma", dict(configs=[(n, W, -0.5, Pl)])),
        (ARG, "sigma", dict(configs=[(n, W, np.inf, Pl)])), (ARG, "sigma", dict(configs=[(n, W, np.nan, Pl)])),
        (ARG, "Pl[0][3]", dict(configs=[(n, W, sg, pl_with(3, -0.1))])),
        (ARG, "Pl[0][5]", dict(configs=[(n, W, sg, pl_with(5, np.inf))])),
        (ARG, "P_c = 0 for column block 1", dict(configs=[(n, W, sg, pl_with(slice(8, 16), 0.0))])),
        (ARG, "T < 1", dict(T=0)), (ARG, "S < 1", dict(S=0)), (ARG, "B < 1", dict(B=0)),
        (ARG, "Rmax", dict(Rmax=W.shape[0] - 1)), (ARG, "Cmax", dict(Cmax=W.shape[1] - 1)),
        (ARG, "flags", dict(flags=2)),
        (ARG, "seeds and U", dict(seeds=seeds)),  # both
        (ARG, "seeds and U", dict(U=None)),  # neither
        (ARG, "configuration 1: R = 5 does not divide n", dict(configs=[(n, W, sg, Pl), (161, W, sg, Pl)])),
    ]
    for status, what, change in bad:
        kw = dict(L=L, M=M, configs=[(n, W, sg, Pl)], T=T, S=S, seeds=None, U=U)
        kw.update(change)
        rc, msg, untouched, _ = _raw(lib_gpu, **kw)
        assert rc == status, (what, rc, msg)
        assert msg.startswith("sa_sc_se:") and what in msg, (what, msg)
        assert untouched, what
    # the Python layer raises them
    with pytest.raises(sp.SparcAmpArgumentError, match="sigma"):
        sp.sc_state_evolution(Pl, M, n, W, 0.0, T, draws=U)
    with pytest.raises(sp.SparcAmpArgumentError, match="does not divide n"):
        sp.sc_state_evolution(Pl, M, n + 1, W, sg, T, draws=U)
    with pytest.raises(sp.SparcAmpError) as ei:
        sp.sc_state_evolution(np.ones(2), scc.MAX_M + 1, 24, np.ones((1, 1)), 0.5, 1, samples=1)
    assert ei.value.code == UNS
    with pytest.raises(sp.SparcAmpError) as ei:
        sp.sc_state_evolution(np.ones(4), M, 2 * big, np.ones((big, 1)), 0.5, 1, samples=1)
    assert ei.value.code == UNS
    with pytest.raises(ValueError):
        sp.sc_state_evolution(Pl, M, n, W, sg, T, draws=U[:, :-1])
    with pytest.raises(ValueError):
        sp.sc_state_evolution(np.stack([Pl, Pl]), M, n, [W], sg, T, draws=U)
    # M need not be a power of two
    assert sp.sc_state_evolution(Pl, 48, n, W, sg, T, samples=S).phi.shape == (T + 1, W.shape[0])


def test_binding_matches_the_header(lib_gpu):
    from sparc_ldpc_amd import _lib
    assert "sa_sc_se" in _lib.EXPORTS and hasattr(lib_gpu, "sa_sc_se") and _lib.SA_SCSE_NO_SKIP == 1
    assert scc.MAX_BLOCKS == _lib.SA_SC_MAX_BLOCKS and se_cases.MAX_M == _lib.SA_SE_MAX_M
