"""CPU: the host rules of the coupled decoder's tolerance stop and frozen column
blocks (csrc/sa_sc.h: sc_wave_plan, sc_check_wave) through the stand-alone
checker `sa_host_check scwave` on the shapes of tests/sc_wave_cases.py in both
precisions: the instance that runs, the extra workspace, and every refusal.
The `sc` mode's output is what it was."""
import json
import os
import subprocess

import numpy as np
import pytest

import sc_wave_cases as wc
from sparc_ldpc_amd._lib import SA_ERR_ARG, SA_PREC_F32, SA_PREC_F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
PRECS = [(SA_PREC_F32, "f32", 4, np.float32), (SA_PREC_F64, "f64", 8, np.float64)]


def scwave(case, prec, B, T, stop_tol, freeze_tol, want_live):
    W = np.asarray(case.W, dtype=np.float64)
    args = [case.L, case.M, case.n, prec, case.R, case.C, B, T]
    p = subprocess.run([CHECKER, "scwave"] + [str(v) for v in args] + [repr(float(stop_tol)), repr(float(freeze_tol)),
                       str(int(want_live))] + [repr(float(v)) for v in W.reshape(-1)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


def expected_E(M):
    E = 1
    while E * 64 < M:
        E *= 2
    return E


@pytest.mark.parametrize("prec,pname,size,dt", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("w", wc.WAVE_CASES, ids=lambda w: w.name)
def test_plan_of_the_table_shapes(w, prec, pname, size, dt):
    c = w.case
    B, T = 8, wc.T
    d = scwave(c, prec, B, T, w.stop_tol, w.freeze_tol, True)
    assert "error" not in d, d
    E = expected_E(c.M)
    assert d["wave"] == 1 and d["instance"] == f"k_scsec_wave<{pname}, {E}>" and d["E"] == E
    assert d["late_loads"] == 1
    # the tolerances in the working precision, as the statement takes them
    assert d["stop_tol"] == float(dt(w.stop_tol)) and d["freeze_tol"] == float(dt(w.freeze_tol))
    assert d["taul_bytes"] == B * 2 * c.C * size
    assert d["live_bytes"] == B * T * c.C
    assert d["grid"] == [c.C * -(-(c.L // c.C) // 4), B] and d["block"] == 256
    assert d["sec_lds"] <= d["lds_limit"]
    # no trace asked for: none sized
    d2 = scwave(c, prec, B, T, w.stop_tol, w.freeze_tol, False)
    assert d2["live_bytes"] == 0 and d2["taul_bytes"] == d["taul_bytes"] and d2["instance"] == d["instance"]
    # the stop alone: the wave form with the table loads where they were
    d3 = scwave(c, prec, B, T, w.stop_tol, 0.0, True)
    assert d3["wave"] == 1 and d3["late_loads"] == 0 and d3["freeze_tol"] == 0
    # the freeze alone
    d4 = scwave(c, prec, 1, 1, 0.0, w.freeze_tol, True)
    assert d4["wave"] == 1 and d4["late_loads"] == 1 and d4["stop_tol"] == 0 and d4["live_bytes"] == c.C


@pytest.mark.parametrize("prec,pname,size,dt", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("w", wc.WAVE_CASES, ids=lambda w: w.name)
def test_zero_tolerances_choose_todays_instances(w, prec, pname, size, dt):
    c = w.case
    for want_live in (False, True):
        d = scwave(c, prec, 8, wc.T, 0.0, 0.0, want_live)
        assert d["wave"] == 0 and d["instance"] == f"k_scsec<{pname}, {expected_E(c.M)}>"
        assert d["taul_bytes"] == 0 and d["live_bytes"] == 0 and d["late_loads"] == 0
    # the same layout as the wave form's: one LDS image, one grid
    assert {k: d[k] for k in ("sec_lds", "grid", "G", "gpc")} == \
        {k: scwave(c, prec, 8, wc.T, 0.01, 0.05, True)[k] for k in ("sec_lds", "grid", "G", "gpc")}


def test_a_tolerance_that_rounds_to_zero_in_binary32_is_off():
    c = wc.BY_NAME["D"].case
    d = scwave(c, SA_PREC_F32, 1, 4, 1e-60, 1e-60, False)
    assert d["wave"] == 0 and d["instance"].startswith("k_scsec<f32")
    d = scwave(c, SA_PREC_F64, 1, 4, 1e-60, 0.0, False)
    assert d["wave"] == 1 and d["stop_tol"] == 1e-60


BAD = [("negative", -1e-3), ("nan", float("nan")), ("inf", float("inf")), ("-inf", -float("inf"))]


@pytest.mark.parametrize("prec", [SA_PREC_F32, SA_PREC_F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,bad", BAD, ids=[b[0] for b in BAD])
@pytest.mark.parametrize("which", ["stop_tol", "freeze_tol"])
def test_refusals(which, name, bad, prec):
    c = wc.BY_NAME["C"].case
    st, ft = (bad, 0.05) if which == "stop_tol" else (0.01, bad)
    d = scwave(c, prec, 2, 8, st, ft, True)
    assert d.get("error") == SA_ERR_ARG, d
    assert which in d["message"] and "finite and non-negative" in d["message"]


def test_a_tolerance_past_binary32_is_refused_there_only():
    c = wc.BY_NAME["C"].case
    d = scwave(c, SA_PREC_F32, 2, 8, 1e300, 0.0, True)
    assert d.get("error") == SA_ERR_ARG and "stop_tol" in d["message"]
    assert scwave(c, SA_PREC_F64, 2, 8, 1e300, 0.0, True)["wave"] == 1


def test_a_refused_layout_is_reported_first():
    c = wc.BY_NAME["C"].case
    W = c.W.copy()
    W[0, 0] = -1.0
    args = [c.L, c.M, c.n, SA_PREC_F32, c.R, c.C, 1, 4, "0.01", "0.05", 1]
    p = subprocess.run([CHECKER, "scwave"] + [str(v) for v in args] + [repr(float(v)) for v in W.reshape(-1)],
                       capture_output=True, text=True, timeout=60)
    d = json.loads(p.stdout)
    assert p.returncode == 0 and d["error"] == SA_ERR_ARG and "W[0,0] is negative" in d["message"]


def test_the_sc_mode_prints_what_it_printed():
    # the keys of the `sc` layout object, in order: tests/test_sc_host.py reads them; none added, none gone
    c = wc.BY_NAME["D"].case
    p = subprocess.run([CHECKER, "sc"] + [str(v) for v in (c.L, c.M, c.n, SA_PREC_F32, c.R, c.C)] +
                       [repr(float(v)) for v in c.W.reshape(-1)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    assert list(json.loads(p.stdout)) == ["R", "C", "L", "M", "n", "n_r", "L_c", "gpc", "G", "zpb", "NZ", "own_fwd", "w", "nhi",
                                          "E", "sec_lds", "lds_limit", "max_blocks", "groups", "zparts"]
