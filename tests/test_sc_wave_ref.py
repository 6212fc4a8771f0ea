"""CPU: the NumPy statement of the coupled decoder's tolerance stop and frozen
column blocks (tests/sc_wave_ref.py) and the table built on it
(tests/sc_wave_cases.py, scripts/sc_wave_case_seeds.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sc_cases
import sc_ref
import sc_wave_cases as wc
import sc_wave_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{w.name}-{s}" for w, s in wc.TABLE]

_RUNS = {}


def runs(w, seed):
    """The float32 and float64 runs of a table entry: computed once, never changed."""
    key = (w.name, seed)
    if key not in _RUNS:
        c = w.case
        _, y = c.rep(seed)
        _RUNS[key] = {dt: ref.amp_sc_wave(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, w.stop_tol, w.freeze_tol, dtype=dt)
                      for dt in (np.float32, np.float64)}
    return _RUNS[key]


@pytest.mark.parametrize("case,seed", sc_cases.TRAJ, ids=lambda v: getattr(v, "name", str(v)))
@pytest.mark.parametrize("early_stop", [True, False])
def test_at_zero_tolerances_the_statement_is_sc_ref(case, seed, early_stop):
    _, y = case.rep(seed)
    T = 24
    b0, s0, p0, n0 = sc_ref.amp_sc(y, case.Pl, case.W, case.L, case.M, T, case.A, early_stop=early_stop)
    b1, s1, p1, live, n1, margin = ref.amp_sc_wave(y, case.Pl, case.W, case.L, case.M, T, case.A, early_stop=early_stop)
    assert b1.dtype == np.float64
    assert np.array_equal(b0, b1) and s0 == s1 and np.array_equal(p0, p1)
    assert sorted(n0) == sorted(n1) and all(np.array_equal(n0[t], n1[t]) for t in n0)
    assert margin == np.inf  # no comparison against a tolerance was made
    assert (live[:s1] == 1).all() and (live[s1:] == 0).all()


def test_the_table_has_the_cases_it_must():
    shapes = {(w.case.L, w.case.M, w.case.n, w.case.omega, w.case.Lambda) for w in wc.WAVE_CASES}
    D, C, F = sc_cases.D, sc_cases.C, sc_cases.FLAT
    assert (D.L, D.M, D.n, D.omega, D.Lambda) in shapes and (C.L, C.M, C.n, C.omega, C.Lambda) in shapes
    assert (64, 32, 340, 2, 16) in shapes and (60, 16, 264, 3, 20) in shapes
    assert (F["L"], F["M"], F["n"], 1, 1) in shapes and np.array_equal(wc.FLAT.W, np.ones((1, 1)))
    assert (wc.LONG.R, wc.LONG.n // wc.LONG.R, wc.LONG.L // wc.LONG.C) == (17, 20, 4)
    assert wc.PAD.L // wc.PAD.C == 3 and sc_cases.C.L // sc_cases.C.C == 5
    tols = {(w.stop_tol, w.freeze_tol) for w in wc.WAVE_CASES}
    assert (0.01, 0.05) in tols and (1e-3, 1e-2) in tols
    assert wc.T <= 40 and all(w.min_margin >= 0.02 and len(w.seeds) == w.nseeds for w in wc.WAVE_CASES)
    # at least one entry thaws a frozen block again
    assert sum(w.recorded(s)["unfreeze"] for w, s in wc.TABLE) >= 1


@pytest.mark.parametrize("w,seed", wc.TABLE, ids=IDS)
def test_recorded_figures_reproduce(w, seed):
    r = runs(w, seed)
    rec = w.recorded(seed)
    _, s32, _, l32, _, m32 = r[np.float32]
    _, s64, _, l64, _, m64 = r[np.float64]
    assert s64 == rec["stop"] < wc.T
    assert ref.frozen_count(l64, s64) == (rec["frozen"], rec["total"]) and rec["frozen"] >= 1
    assert ref.unfreeze_events(l64, s64) == rec["unfreeze"]
    assert round(m32, 6) == rec["margin32"] and round(m64, 6) == rec["margin64"]
    assert min(m32, m64) >= w.min_margin
    # float32 and float64 agree on every mask and on the stop index
    assert s32 == s64 and np.array_equal(l32, l64)
    assert r[np.float32][0].dtype == np.float32 and r[np.float32][2].dtype == np.float32


@pytest.mark.parametrize("w,seed", wc.TABLE, ids=IDS)
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_frozen_block_keeps_its_beta(w, seed, dt):
    beta, stop, phi, live, snaps, _ = runs(w, seed)[dt]
    c = w.case
    assert (live[0] == 1).all()  # t = 0: every block is live
    assert sorted(snaps) == list(range(stop + 1)) and np.array_equal(snaps[stop], beta)
    changed = 0
    for t in range(stop):
        a, b = snaps[t].reshape(c.C, -1), snaps[t + 1].reshape(c.C, -1)
        for cb in range(c.C):
            if not live[t, cb]:
                assert np.array_equal(a[cb], b[cb]), (t, cb)
            else:
                changed += not np.array_equal(a[cb], b[cb])
    assert changed > 0
    assert (phi[:stop] > 0).all() and (phi[stop:] == 0).all() and (live[stop:] == 0).all()


def test_an_unfreeze_event_is_a_drift_past_the_tolerance():
    """Nothing is sticky: in the entry with the most unfreeze events, a block that thaws does so because
    its tau_c^2 has left taul_c, the value of its last live iteration, by more than freeze_tol."""
    w, seed = max(wc.TABLE, key=lambda e: e[0].recorded(e[1])["unfreeze"])
    assert w.recorded(seed)["unfreeze"] >= 1
    _, stop, phi, live, _, _ = runs(w, seed)[np.float64]
    c = w.case
    tau2 = c.R / (c.W[None, :, :] / phi[:stop, :, None]).sum(axis=1)   # (stop, C)
    events = 0
    for cb in range(c.C):
        taul = tau2[0, cb]
        for t in range(1, stop):
            drift = abs(tau2[t, cb] - taul) > w.freeze_tol * taul
            assert bool(live[t, cb]) == bool(drift), (t, cb)
            events += bool(live[t, cb]) and not live[t - 1, cb]
            if live[t, cb]:
                taul = tau2[t, cb]
    assert events == w.recorded(seed)["unfreeze"]


def test_stop_off_keeps_freezing():
    w, seed = wc.BY_NAME["LONG"], 3
    c = w.case
    _, y = c.rep(seed)
    on = runs(w, seed)[np.float64]
    off = ref.amp_sc_wave(y, c.Pl, c.W, c.L, c.M, wc.T, c.A, w.stop_tol, w.freeze_tol, early_stop=False)
    assert off[1] == wc.T and np.array_equal(off[3][:on[1]], on[3][:on[1]])
    assert (off[3][on[1]:] == 0).any() and np.array_equal(off[4][on[1]], on[0])


def test_the_seed_script_rejects_what_the_margins_forbid_and_reproduces_the_table():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import sc_wave_case_seeds as pick
    finally:
        sys.path.pop(0)
    # the (0.01, 0.05) reps whose nearest comparison is under 0.02 from flipping
    for name, seed in (("LONG", 1), ("PAD", 2), ("PAD", 3)):
        rec, why = pick.look(wc.BY_NAME[name], seed)
        assert why is not None and "margin" in why and min(rec["margin32"], rec["margin64"]) < 0.02, (name, seed, rec)
    for w, seed in wc.TABLE:
        rec, why = pick.look(w, seed)
        assert why is None and rec == w.recorded(seed)
    # the first seeds from 0: every smaller seed of a case was passed over
    for w in wc.WAVE_CASES:
        for seed in range(max(w.seeds)):
            assert (seed in w.seeds) == (pick.look(w, seed)[1] is None), (w.name, seed)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sc_wave_case_seeds.py"), "--help"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0 and "--write" in p.stdout
