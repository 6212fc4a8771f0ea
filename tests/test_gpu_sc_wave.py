"""GPU: the coupled decoder's opt-in tolerance stop and frozen column blocks
(sa_sc_amp_ex / sa_sc_mc_ex, the wave form of k_scsec)
against the NumPy statement tests/sc_wave_ref.py on the table of
tests/sc_wave_cases.py, in both precisions.  Live masks and stop indices are
held to the statement by equality (the table's seeds keep every comparison at
least MIN_MARGIN from flipping), beta and the phi trace to test_gpu_sc.py's
bars (1e-5 / 1e-11), both norm-relative.  The largest per-entry deviation of
the phi trace is printed beside it and not asserted: over a run to the stop it
is no binary32 property (the float32 run of the NumPy statement itself is up to
1.1e-5 per entry from the float64 one on this table, 5.6e-7 in norm)."""
import ctypes as ct

import numpy as np
import pytest

import sc_wave_cases as wc
import sc_wave_ref as ref
from test_gpu_sc import PRECS, TOL, rel

pytestmark = pytest.mark.gpu

D = ct.POINTER(ct.c_double)
I = ct.POINTER(ct.c_int)
I32 = ct.POINTER(ct.c_int32)
U8 = ct.POINTER(ct.c_ubyte)
BAD_TOLS = [(-1e-3, "negative"), (float("nan"), "nan"), (float("inf"), "inf"), (-float("inf"), "-inf")]


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd as s
    return s


_OPS = {}


def transforms(sp, case, prec):
    key = (case.name, prec)
    if key not in _OPS:
        Ab, Az, ordering = sp.sc_transforms(case.L, case.M, case.n, case.W, precision=prec, device=0)
        assert np.array_equal(ordering, case.ordering)
        _OPS[key] = (Ab, Az)
    return _OPS[key]


_REF = {}


def reference(w, seed, early_stop=True):
    """The binary64 statement's run of a table entry, T = 40: computed once, never changed."""
    key = (w.name, seed, early_stop)
    if key not in _REF:
        c = w.case
        _, y = c.rep(seed)
        beta, stop, phi, live, snaps, margin = ref.amp_sc_wave(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, w.stop_tol, w.freeze_tol,
                                                               early_stop=early_stop)
        for v in list(snaps.values()) + [phi, live, y]:
            v.setflags(write=False)
        _REF[key] = (y, stop, phi, live, snaps, margin)
    return _REF[key]


def run(sp, w, prec, y, T, **kw):
    Ab, _ = transforms(sp, w.case, prec)
    return sp.amp_sc_batch(np.asarray(y).reshape(-1, w.case.n), w.case.Pl, T, Ab, stop_tol=w.stop_tol,
                           freeze_tol=w.freeze_tol, return_live=True, **kw)


IDS = [f"{w.name}-{s}" for w, s in wc.TABLE]


# ---- 1. (0, 0) is sa_sc_amp ---------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nb", [1, 3])
def test_ex_at_zero_is_sa_sc_amp(sp, lib_gpu, prec, nb):
    w = wc.BY_NAME["D"]
    c = w.case
    Ab, _ = transforms(sp, c, prec)
    ys = np.ascontiguousarray(np.stack([c.rep(s)[1] for s in (1, 2, 3)[:nb]]))
    T = 12
    sc = Ab.op._sc
    b0, b1 = np.full((nb, c.L * c.M), 7.0), np.full((nb, c.L * c.M), 8.0)
    i0, i1 = np.full(nb, -5, dtype=np.int32), np.full(nb, -6, dtype=np.int32)
    p0, p1 = np.full((nb, T, c.R), 7.0), np.full((nb, T, c.R), 8.0)
    live = np.full((nb, T, c.C), 9, dtype=np.uint8)
    assert lib_gpu.sa_sc_amp(sc, nb, ys.ctypes.data_as(D), c.Pl.ctypes.data_as(D), T, b0.ctypes.data_as(D), i0.ctypes.data_as(I),
                             p0.ctypes.data_as(D), 0) == 0
    assert lib_gpu.sa_sc_amp_ex(sc, nb, ys.ctypes.data_as(D), c.Pl.ctypes.data_as(D), T, 0.0, 0.0, b1.ctypes.data_as(D),
                                i1.ctypes.data_as(I), p1.ctypes.data_as(D), live.ctypes.data_as(U8), 0) == 0
    assert np.array_equal(b0, b1) and np.array_equal(i0, i1) and np.array_equal(p0, p1)
    assert (i0 < T).all()  # the stop was taken, so the rows behind it are there to check
    assert np.array_equal(live, (np.arange(T)[None, :, None] < i0[:, None, None]).astype(np.uint8) * np.ones((1, 1, c.C), np.uint8))
    # and through Python: the keywords at their defaults, and at zero with the trace
    beta, iters, phi = sp.amp_sc_batch(ys, c.Pl, T, Ab)
    beta2, iters2, phi2, live2 = sp.amp_sc_batch(ys, c.Pl, T, Ab, stop_tol=0.0, freeze_tol=0.0, return_live=True)
    assert np.array_equal(beta, b0) and np.array_equal(iters, i0) and np.array_equal(phi, p0)
    assert np.array_equal(beta2, b0) and np.array_equal(iters2, i0) and np.array_equal(phi2, p0) and np.array_equal(live2, live)


# ---- 2. every table entry against the statement ----------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("w,seed", wc.TABLE, ids=IDS)
def test_table_entry(sp, w, seed, prec):
    y, stop, phi_ref, live_ref, snaps, margin = reference(w, seed)
    rec = w.recorded(seed)
    assert stop == rec["stop"] and stop < wc.T and margin >= w.min_margin
    for T in (1, 2, 4, 8, wc.T):
        beta, iters, phi, live = run(sp, w, prec, y, T)
        ran = min(stop, T)
        assert live.shape == (1, T, w.case.C) and live.dtype == np.uint8
        e_b = rel(beta, snaps[ran])
        e_p = rel(phi[0, :ran], phi_ref[:ran])
        e_pe = np.abs(phi[0, :ran] / phi_ref[:ran] - 1).max()
        print(f"{w.name} seed {seed} {prec} T={T}: stop {int(iters[0])} ({ran}) beta {e_b:.2e} phi {e_p:.2e} "
              f"(per entry {e_pe:.2e}) frozen {int(w.case.C * ran - live[0].sum())}")
        assert np.array_equal(live[0], live_ref[:T]), (T, np.argwhere(live[0] != live_ref[:T]))
        assert iters[0] == ran
        assert np.all(phi[0, ran:] == 0) and np.all(live[0, ran:] == 0)
        assert e_b <= TOL[prec], (T, e_b)
        assert e_p <= TOL[prec], (T, e_p)
    frozen, total = ref.frozen_count(live[0], int(iters[0]))
    assert (frozen, total) == (rec["frozen"], rec["total"])


# ---- 3. a frozen block's beta stays, bit for bit -----------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("w,seed", wc.TABLE, ids=IDS)
def test_frozen_block_keeps_its_beta(sp, w, seed, prec):
    y, stop, _, live_ref, _, _ = reference(w, seed)
    c = w.case
    ts, cs = np.nonzero(live_ref[:stop] == 0)
    assert ts.size, "the table's entries freeze a block before the stop"
    t = int(ts[0])
    frozen = np.nonzero(live_ref[t] == 0)[0]
    b0 = run(sp, w, prec, y, t)[0].reshape(c.C, -1)
    b1, it1, _, live = run(sp, w, prec, y, t + 1)
    b1 = b1.reshape(c.C, -1)
    assert it1[0] == t + 1 and np.array_equal(live[0, t], live_ref[t])
    for cb in frozen:
        assert np.array_equal(b0[cb], b1[cb]), (t, cb)
    if len(frozen) < c.C:
        assert not np.array_equal(b0, b1)  # the live blocks were computed


# ---- 4. two runs; a codeword alone and in a mixed batch ---------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_runs_and_batches_are_equal_bit_for_bit(sp, prec):
    w = wc.BY_NAME["LONG"]
    c = w.case
    ys = np.stack([c.rep(s)[1] for s in (2, 3, 6)])
    a = run(sp, w, prec, ys, wc.T)
    b = run(sp, w, prec, ys, wc.T)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    beta, iters, phi, live = a
    # the batch is mixed: different stop indices and different masks
    assert len(set(int(i) for i in iters)) > 1
    assert not np.array_equal(live[0], live[1]) and not np.array_equal(live[1], live[2])
    for k in range(3):
        b1, i1, p1, l1 = run(sp, w, prec, ys[k], wc.T)
        assert np.array_equal(b1[0], beta[k]) and i1[0] == iters[k] and np.array_equal(p1[0], phi[k])
        assert np.array_equal(l1[0], live[k])
    # the single-codeword form
    Ab, Az = transforms(sp, c, prec)
    b1, l1 = sp.amp_sc(ys[0], c.Pl, c.L, c.M, wc.T, Ab, Az, stop_tol=w.stop_tol, freeze_tol=w.freeze_tol, return_live=True)
    assert np.array_equal(b1.reshape(-1), beta[0]) and np.array_equal(l1, live[0])
    assert np.array_equal(sp.amp_sc(ys[0], c.Pl, c.L, c.M, wc.T, Ab, Az, stop_tol=w.stop_tol, freeze_tol=w.freeze_tol), b1)


# ---- 5. SA_FLAG_NO_EARLY_STOP -------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_no_early_stop_still_freezes(sp, prec):
    w, seed = wc.BY_NAME["LONG"], 3
    c = w.case
    y, stop, phi_ref, live_ref, snaps, margin = reference(w, seed, early_stop=False)
    # the statement with the stop off: its freeze decisions are as far from flipping, in both precisions
    _, s32, _, l32, _, m32 = ref.amp_sc_wave(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, w.stop_tol, w.freeze_tol, early_stop=False,
                                             dtype=np.float32)
    assert stop == s32 == wc.T and np.array_equal(l32, live_ref) and min(margin, m32) >= w.min_margin
    T = 20
    beta, iters, phi, live = run(sp, w, prec, y, T, early_stop=False)
    assert iters[0] == T and np.all(phi[0] > 0)
    assert np.array_equal(live[0], live_ref[:T])
    assert live[0, w.recorded(seed)["stop"]:].sum() < c.C * (T - w.recorded(seed)["stop"])  # frozen behind the stop index too
    print(f"no early stop {prec}: beta {rel(beta, snaps[T]):.2e}")
    assert rel(beta, snaps[T]) <= TOL[prec]


# ---- 6. Monte Carlo -----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_mc_with_tolerances_equals_batch_decode_of_the_same_draws(sp, prec):
    from sparc_ldpc_amd.harness import _draw_reps
    w = wc.BY_NAME["LONG"]
    c = w.case
    Ab, _ = transforms(sp, c, prec)
    seeds = list(range(8))
    kw = dict(stop_tol=w.stop_tol, freeze_tol=w.freeze_tol)
    errs, its, dec, live = sp.mc_decode_sc(Ab, c.Pl, c.sigma, wc.T, seeds, batch=3, return_live=True, **kw)
    errs2, its2, dec2 = sp.mc_decode_sc(Ab, c.Pl, c.sigma, wc.T, seeds, batch=8, **kw)
    idx, noise = _draw_reps(seeds, c.L, c.M, c.n, c.sigma)
    beta0 = np.zeros((8, c.L * c.M))
    cl = np.sqrt(c.n * c.Pl)
    for k in range(8):
        beta0[k, np.arange(c.L) * c.M + idx[k]] = cl
    y = Ab.op.Ab_batch(beta0) + noise
    beta, iters, _, live_b = sp.amp_sc_batch(y, c.Pl, wc.T, Ab, return_live=True, **kw)
    want = beta.reshape(8, c.L, c.M).argmax(axis=2)
    werr = np.array([sum(bin(int(v)).count("1") for v in (want[k] ^ idx[k])) for k in range(8)])
    assert dec.dtype == its.dtype == errs.dtype == np.int32 and live.dtype == np.uint8
    assert np.array_equal(dec, want) and np.array_equal(its, iters) and np.array_equal(errs, werr)
    assert np.array_equal(live, live_b) and live.sum() < live_b.size
    assert np.array_equal(dec2, want) and np.array_equal(its2, iters) and np.array_equal(errs2, werr)
    # the operator's own call, without the trace
    d3, i3, e3, ms = Ab.op.mc(idx, noise, c.Pl, wc.T, **kw)
    assert np.array_equal(d3, want) and np.array_equal(i3, iters) and np.array_equal(e3, werr) and ms > 0
    # the tolerances were in force: the stop indices are not those of the decode without them
    _, its0, _ = sp.mc_decode_sc(Ab, c.Pl, c.sigma, wc.T, seeds, batch=8)
    assert not np.array_equal(its0, its)


# ---- 7. the C calls: a null live_out, refusals ------------------------------------------------------------
def _amp_ex(lib, sc, c, y, T, st, ft, bout, live=None, iters=None, flags=0):
    return lib.sa_sc_amp_ex(sc, 1, y.ctypes.data_as(D), c.Pl.ctypes.data_as(D), T, st, ft, bout.ctypes.data_as(D),
                            None if iters is None else iters.ctypes.data_as(I), None,
                            None if live is None else live.ctypes.data_as(U8), flags)


def test_null_live_out_is_accepted(sp, lib_gpu):
    w, seed = wc.BY_NAME["PAD"], 1
    c = w.case
    Ab, _ = transforms(sp, c, "fp32")
    y = np.ascontiguousarray(c.rep(seed)[1])
    b0, b1 = np.full(c.L * c.M, 7.0), np.full(c.L * c.M, 8.0)
    live = np.full((wc.T, c.C), 9, dtype=np.uint8)
    i0 = np.full(1, -5, dtype=np.int32)
    assert _amp_ex(lib_gpu, Ab.op._sc, c, y, wc.T, w.stop_tol, w.freeze_tol, b0) == 0
    assert _amp_ex(lib_gpu, Ab.op._sc, c, y, wc.T, w.stop_tol, w.freeze_tol, b1, live, i0) == 0
    assert np.array_equal(b0, b1) and i0[0] == w.recorded(seed)["stop"] and live.max() == 1
    rs = np.random.RandomState(seed)
    idx = np.ascontiguousarray(rs.randint(0, c.M, (1, c.L)), dtype=np.int32)
    noise = rs.randn(1, c.n) * c.sigma
    d0, d1 = np.full((1, c.L), -1, dtype=np.int32), np.full((1, c.L), -2, dtype=np.int32)
    for dec, lv in ((d0, None), (d1, live.ctypes.data_as(U8))):
        assert lib_gpu.sa_sc_mc_ex(Ab.op._sc, 1, idx.ctypes.data_as(I32), noise.ctypes.data_as(D), c.Pl.ctypes.data_as(D), wc.T,
                                   w.stop_tol, w.freeze_tol, 0, dec.ctypes.data_as(I32), None, None, lv, None) == 0
    assert np.array_equal(d0, d1) and d0.min() >= 0


@pytest.mark.parametrize("bad,name", BAD_TOLS, ids=[n for _, n in BAD_TOLS])
@pytest.mark.parametrize("which", ["stop_tol", "freeze_tol"])
def test_refusals_through_c_and_python(sp, lib_gpu, which, bad, name):
    w = wc.BY_NAME["C"]
    c = w.case
    Ab, Az = transforms(sp, c, "fp32")
    sc = Ab.op._sc
    st, ft = (bad, 0.05) if which == "stop_tol" else (0.01, bad)
    y = np.ascontiguousarray(c.rep(0)[1])
    bout = np.full(c.L * c.M, 7.0)
    live = np.full((4, c.C), 9, dtype=np.uint8)
    iters = np.full(1, -5, dtype=np.int32)
    rc = _amp_ex(lib_gpu, sc, c, y, 4, st, ft, bout, live, iters)
    msg = lib_gpu.sa_last_error().decode()
    assert rc == sp._lib.SA_ERR_ARG and msg.startswith("sa_sc_amp_ex:") and which in msg, (rc, msg)
    assert (bout == 7.0).all() and (live == 9).all() and iters[0] == -5
    idx = np.zeros((1, c.L), dtype=np.int32)
    dec = np.full((1, c.L), -1, dtype=np.int32)
    errs = np.full(1, -5, dtype=np.int32)
    ms = np.full(1, 7.0)
    rc = lib_gpu.sa_sc_mc_ex(sc, 1, idx.ctypes.data_as(I32), None, c.Pl.ctypes.data_as(D), 4, st, ft, 0, dec.ctypes.data_as(I32),
                             iters.ctypes.data_as(I32), errs.ctypes.data_as(I32), live.ctypes.data_as(U8), ms.ctypes.data_as(D))
    msg = lib_gpu.sa_last_error().decode()
    assert rc == sp._lib.SA_ERR_ARG and msg.startswith("sa_sc_mc_ex:") and which in msg, (rc, msg)
    assert (dec == -1).all() and iters[0] == -5 and errs[0] == -5 and (live == 9).all() and ms[0] == 7.0
    kw = dict(stop_tol=st, freeze_tol=ft)
    for call in (lambda: Ab.op.amp_batch(y, c.Pl, 4, **kw), lambda: Ab.op.mc(idx, None, c.Pl, 4, **kw),
                 lambda: sp.amp_sc_batch(y.reshape(1, -1), c.Pl, 4, Ab, **kw),
                 lambda: sp.amp_sc(y, c.Pl, c.L, c.M, 4, Ab, Az, **kw),
                 lambda: sp.mc_decode_sc(Ab, c.Pl, c.sigma, 4, [0, 1], **kw)):
        with pytest.raises(sp._lib.SparcAmpArgumentError, match=which):
            call()


def test_unknown_flags_and_exports(sp, lib_gpu):
    from sparc_ldpc_amd import _lib
    assert "sa_sc_amp_ex" in _lib.EXPORTS and "sa_sc_mc_ex" in _lib.EXPORTS
    assert lib_gpu.sa_version() >= b"sparc_amp 0.5"
    c = wc.BY_NAME["C"].case
    Ab, _ = transforms(sp, c, "fp32")
    bout = np.full(c.L * c.M, 7.0)
    y = np.zeros(c.n)
    assert _amp_ex(lib_gpu, Ab.op._sc, c, y, 4, 0.01, 0.05, bout, flags=64) == _lib.SA_ERR_ARG
    assert b"sa_sc_amp_ex: unknown flags" in lib_gpu.sa_last_error() and (bout == 7.0).all()
