"""GPU: state evolution on the device (sa_se / sa_se_draws, csrc/sa_se.hip;
sparc_ldpc_amd.se) against its NumPy statement (tests/se_ref.py) on the cases
of tests/se_cases.py.

Tolerance: per case, 64 x the largest gap between the statement in binary64
and in np.longdouble (recorded by scripts/se_case_seeds.py from the statement
alone), absolute, for tau2, x and sections: room for the device library's exp
(within an ulp of the host's) and the wave-tree summation order against
NumPy's.  The miss counts must be equal: every case's seed was chosen so that
each miss comparison has a relative margin of at least 1e-9.

The draws' bar, 2**-49 relative, is the one tests/test_gpu_mc_draws.py
derives for the same generator (a few values differ, by the two logs)."""
import ctypes as ct

import numpy as np
import pytest

import se_cases as sc

pytestmark = pytest.mark.gpu

BAR = 2.0 ** -49
NAMES = list(sc.CASES)


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_RUNS = {}


def _host_rows_run(sp, name):
    """The device's result on the case's NumPy rows, computed once."""
    if name not in _RUNS:
        c = sc.case(name)
        _RUNS[name] = sp.state_evolution(c.Pl, c.M, c.n, c.sigma, c.T, draws=c.U)
    return _RUNS[name]


def _same_bits(a, b):
    for f in ("tau2", "x", "miss", "sections", "ser"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


@pytest.mark.parametrize("name", NAMES)
def test_against_the_statement(sp, name):
    c = sc.case(name)
    assert c.margin >= sc.MARGIN
    r = _host_rows_run(sp, name)
    assert r.tau2.shape == (c.B, c.T + 1) and r.x.shape == (c.B, c.T) and r.sections.shape == (c.B, c.L)
    d_tau, d_x, d_sec = (float(np.max(np.abs(r.tau2 - c.tau2))), float(np.max(np.abs(r.x - c.x))),
                         float(np.max(np.abs(r.sections - c.E))))
    print(f"{name}: tol {c.tol:.3e}; tau2 {d_tau:.3e}, x {d_x:.3e}, sections {d_sec:.3e}; "
          f"misses {r.miss[:, -1].tolist()} (statement {c.miss[:, -1].tolist()}); {r.ms:.3f} ms")
    np.testing.assert_array_equal(r.miss, c.miss)
    assert d_tau <= c.tol and d_x <= c.tol and d_sec <= c.tol
    np.testing.assert_array_equal(r.ser, c.miss / float(c.L * c.S))


@pytest.mark.parametrize("name", NAMES)
def test_seeded_path(sp, name):
    c = sc.case(name)
    Ud = sp.se_draws(c.seeds, c.M)
    assert Ud.shape == c.U.shape and np.all(np.isfinite(Ud))
    zero = c.U == 0
    ratio = np.abs(Ud - c.U)[~zero] / np.abs(c.U[~zero])
    print(f"{name}: {int((Ud != c.U).sum())} of {Ud.size} drawn values differ from NumPy's, "
          f"largest ratio {ratio.max() * 2.0 ** 52:.3f} * 2**-52")
    assert np.all(Ud[zero] == 0)
    assert ratio.max() <= BAR
    seeded = sp.state_evolution(c.Pl, c.M, c.n, c.sigma, c.T, samples=c.S, seed=c.seed, draws="device")
    _same_bits(seeded, sp.state_evolution(c.Pl, c.M, c.n, c.sigma, c.T, draws=Ud))


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_same_bits(sp, name):
    c = sc.case(name)
    _same_bits(_host_rows_run(sp, name), sp.state_evolution(c.Pl, c.M, c.n, c.sigma, c.T, draws=c.U))


def test_batch_is_its_allocations_alone(sp):
    c = sc.case("batch3")
    r = _host_rows_run(sp, "batch3")
    assert c.B == 3
    for b in range(c.B):
        one = sp.state_evolution(c.Pl[b], c.M, c.n, c.sigma[b], c.T, draws=c.U)
        assert one.tau2.shape == (c.T + 1,)
        for f in ("tau2", "x", "miss", "sections"):
            np.testing.assert_array_equal(getattr(one, f), getattr(r, f)[b], err_msg=f"{f}, allocation {b}")


@pytest.mark.parametrize("name", [k for k in NAMES if sc.CASES[k][0] > 1])
def test_permuted_sections(sp, name):
    c = sc.case(name)
    r = _host_rows_run(sp, name)
    perm = np.random.RandomState(7).permutation(c.L)
    if np.array_equal(perm, np.arange(c.L)):
        perm = perm[::-1]
    rp = sp.state_evolution(c.Pl[:, perm], c.M, c.n, c.sigma, c.T, draws=c.U)
    np.testing.assert_array_equal(rp.miss, r.miss)
    assert np.max(np.abs(rp.tau2 - r.tau2)) <= c.tol
    assert np.max(np.abs(rp.x - r.x)) <= c.tol
    # the same permutation of E_l (to the rounding of tau2 that the classes' new order brings)
    assert np.max(np.abs(rp.sections - r.sections[:, perm])) <= c.tol
    assert np.max(np.abs(rp.sections - c.E[:, perm])) <= c.tol
    # one iteration reads the same tau_0: E_l moves with its section bit for bit
    r1 = sp.state_evolution(c.Pl, c.M, c.n, c.sigma, 1, draws=c.U)
    rp1 = sp.state_evolution(c.Pl[:, perm], c.M, c.n, c.sigma, 1, draws=c.U)
    np.testing.assert_array_equal(rp1.sections, r1.sections[:, perm])


# ---- refusals ---------------------------------------------------------------------

_SENTINEL = -77.25


def _raw(lib, B, L, M, n, Pl, sigma, T, S, seeds=None, U=None):
    """sa_se called as C would, on outputs filled with a sentinel."""
    from sparc_ldpc_amd import _lib
    Pl = np.ascontiguousarray(Pl, dtype=np.float64)
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    nb, nt = max(B, 1), max(T, 1)
    outs = [np.full((nb, nt + 1), _SENTINEL), np.full((nb, nt), _SENTINEL), np.full((nb, nt), -77, dtype=np.int64),
            np.full((nb, max(L, 1)), _SENTINEL)]
    ms = ct.c_double(_SENTINEL)
    seeds = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
    U = None if U is None else np.ascontiguousarray(U, dtype=np.float64)
    rc = lib.sa_se(0, B, L, M, n, _lib.dptr(Pl), _lib.dptr(sigma), T, S,
                   None if seeds is None else seeds.ctypes.data_as(ct.POINTER(ct.c_uint32)),
                   None if U is None else _lib.dptr(U), _lib.dptr(outs[0]), _lib.dptr(outs[1]),
                   outs[2].ctypes.data_as(ct.POINTER(ct.c_int64)), _lib.dptr(outs[3]),
                   ct.cast(ct.pointer(ms), ct.POINTER(ct.c_double)))
    untouched = (all(np.all(o == _SENTINEL) for o in (outs[0], outs[1], outs[3])) and np.all(outs[2] == -77)
                 and ms.value == _SENTINEL)
    return rc, lib.sa_last_error().decode(), untouched


def test_refusals(sp, lib_gpu):
    from sparc_ldpc_amd import _lib
    L, M, n, T, S = 4, 8, 12, 3, 5
    Pl = 0.5 * np.ones((1, L))
    sig = np.array([0.6])
    U = np.random.RandomState(1).randn(S, M)
    seeds = np.arange(S)
    rc, msg, untouched = _raw(lib_gpu, 1, L, M, n, Pl, sig, T, S, U=U)
    assert rc == _lib.SA_OK and not untouched
    bad = [  # (what the message must name, arguments)
        ("sigma", dict(sigma=[0.0])), ("sigma", dict(sigma=[-0.5])), ("sigma", dict(sigma=[np.inf])),
        ("sigma", dict(sigma=[np.nan])),
        ("Pl", dict(Pl=np.array([[0.5, -0.1, 0.5, 0.5]]))),
        ("P = sum(Pl) is 0", dict(Pl=np.zeros((1, L)))),
        ("T < 1", dict(T=0)), ("S < 1", dict(S=0)), ("B < 1", dict(B=0)), ("M < 2", dict(M=1)),
        ("seeds and U", dict(seeds=seeds)),  # both
        ("seeds and U", dict(U=None)),  # neither
    ]
    for what, change in bad:
        kw = dict(B=1, L=L, M=M, n=n, Pl=Pl, sigma=sig, T=T, S=S, seeds=None, U=U)
        kw.update(change)
        rc, msg, untouched = _raw(lib_gpu, **kw)
        assert rc == _lib.SA_ERR_ARG, (what, rc, msg)
        assert msg.startswith("sa_se:") and what in msg, (what, msg)
        assert untouched, what
    # one above the largest row: unsupported, nothing written
    big = sc.MAX_M + 1
    rc, msg, untouched = _raw(lib_gpu, 1, 2, big, 24, np.ones((1, 2)), sig, 1, 1, U=np.zeros((1, big)))
    assert rc == _lib.SA_ERR_UNSUPPORTED and "SA_SE_MAX_M" in msg and untouched
    assert _lib.SA_SE_MAX_M == sc.MAX_M
    # the Python layer raises them
    with pytest.raises(sp.SparcAmpArgumentError, match="sigma"):
        sp.state_evolution(Pl[0], M, n, 0.0, T, draws=U)
    with pytest.raises(sp.SparcAmpError) as ei:
        sp.state_evolution(np.ones(2), big, 24, 0.5, 1, samples=1)
    assert ei.value.code == _lib.SA_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sp.state_evolution(Pl[0], M, n, 0.6, T, draws=U[:, :-1])
    with pytest.raises(ValueError, match="Seed must be between 0 and 2\\*\\*32 - 1"):
        sp.se_draws([1, 2 ** 32], M)


# ---- the Python layer ---------------------------------------------------------------

def test_state_evolution_shapes(sp):
    L, M, n, T, S = 6, 16, 24, 5, 9
    Pl = sp.pa_parameterised(L, 1.0, 2.0, 1.0, 0.5)
    r = sp.state_evolution(Pl, M, n, 0.6, T, samples=S, seed=3)
    assert r.tau2.shape == (T + 1,) and r.x.shape == (T,) and r.ser.shape == (T,) and r.sections.shape == (L,)
    assert r.miss.dtype == np.int64 and r.ms > 0
    assert r.tau2[0] == 0.6 * 0.6 + Pl.sum()
    np.testing.assert_array_equal(r.ser, r.miss / float(L * S))
    r2 = sp.state_evolution(np.stack([Pl, Pl[::-1]]), M, n, [0.6, 0.7], T, samples=S, seed=3)
    assert r2.tau2.shape == (2, T + 1) and r2.x.shape == (2, T) and r2.ser.shape == (2, T)
    assert r2.sections.shape == (2, L)
    for f in ("tau2", "x", "ser", "sections"):
        np.testing.assert_array_equal(getattr(r2, f)[0], getattr(r, f), err_msg=f)
    # a scalar sigma serves every allocation
    r3 = sp.state_evolution(np.stack([Pl, Pl]), M, n, 0.6, T, samples=S, seed=3)
    np.testing.assert_array_equal(r3.tau2[1], r.tau2)
    assert sp.se_draws([5, 6, 7], M).shape == (3, M)


def test_pa_search_is_its_single_calls(sp):
    L, M, S, T, P, sigma = 40, 64, 33, 6, 2.0, 0.6
    n = int(L * np.log2(M))
    a_values, f_values = [0.6, 1.2], [0.4, 0.8]
    res = sp.pa_search(L, M, n, P, sigma, a_values, f_values, T, samples=S, seed=2)
    assert res.x.shape == (2, 2) and res.ser.shape == (2, 2) and res.iters.shape == (2, 2)
    C = 0.5 * np.log2(1.0 + P / sigma ** 2)
    xs = np.zeros((2, 2))
    for i, a in enumerate(a_values):
        for j, f in enumerate(f_values):
            one = sp.state_evolution(sp.pa_parameterised(L, C, P, a, f), M, n, sigma, T, samples=S, seed=2)
            assert res.x[i, j] == one.x[-1] and res.ser[i, j] == one.ser[-1]
            first = int(np.argmax(one.ser == one.ser[-1])) + 1
            assert res.iters[i, j] == first and 1 <= first <= T
            xs[i, j] = one.x[-1]
    i, j = np.unravel_index(int(np.argmax(xs)), xs.shape)
    assert res.best == (a_values[i], f_values[j])
