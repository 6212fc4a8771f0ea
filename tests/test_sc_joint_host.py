"""CPU: the host rules of the coupled beta_0 start, the staged coupled context
and the glue on it (csrc/sa_sc.h: sc_decode_launches, sc_stage_rule,
sc_glue_check, the extra workspace) through the stand-alone checker
`sa_host_check scjoint` on the cases of tests/sc_joint_cases.py in both
precisions.  The `sc` and `scwave` modes print what they printed."""
import json
import os
import subprocess

import numpy as np
import pytest

import sc_cases
import sc_joint_cases as jc
import sc_wave_cases as wc
from sparc_ldpc_amd._lib import SA_ERR_ARG, SA_ERR_UNSUPPORTED, SA_PREC_F32, SA_PREC_F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
PRECS = [(SA_PREC_F32, "f32"), (SA_PREC_F64, "f64")]


def run(mode, args):
    p = subprocess.run([CHECKER, mode] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return p.stdout


def scjoint(c, prec, B, T, l0, ns, beta0, stop_tol=0.0, freeze_tol=0.0, calls=(), M=None):
    W = [repr(float(v)) for v in np.asarray(c.W, dtype=np.float64).reshape(-1)]
    return json.loads(run("scjoint", [c.L, c.M if M is None else M, c.n, prec, c.R, c.C, B, T, l0, ns, int(beta0),
                                      repr(float(stop_tol)), repr(float(freeze_tol))] + W + list(calls)))


def case_range(c):
    return (c.l0, c.ns) if c.coded else (0, c.L)


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("c", jc.START_CASES, ids=lambda c: c.name)
def test_the_table_shapes(c, prec, pname):
    B, T = 5, 3
    l0, ns = case_range(c)
    d = scjoint(c, prec, B, T, l0, ns, True)
    assert "error" not in d, d
    lgm = c.lgm
    assert d["lgM"] == lgm and d["l0"] == l0 and d["ns"] == ns
    assert d["rescale"] == (1 if ns < c.L else 0)
    assert d["cd_bytes"] == 8 * c.L and d["glue_stage_bytes"] == 8 * B * ns * lgm
    zpb = -(-(c.n // c.R) // 64)
    assert d["start_grid"] == [c.R * zpb, B] and d["start_block"] == 64 and d["zpb"] == zpb
    assert d["n_r"] == c.n // c.R and d["L_c"] == c.L // c.C and d["own_fwd"] == (1 if (c.L // c.C) % 4 else 0)
    assert d["l0_block"] == l0 // (c.L // c.C) and d["l0_on_block_edge"] == (1 if l0 % (c.L // c.C) == 0 else 0)


def test_what_the_table_reaches():
    d = {c.name: scjoint(c, SA_PREC_F64, 1, 1, *case_range(c), True) for c in jc.START_CASES}
    assert d["K0"]["rescale"] == 0 and d["K0"]["l0"] == 0 and d["K0"]["n_r"] == 32
    assert d["K1"]["l0"] == 16 and d["K1"]["l0_on_block_edge"] == 1 and d["K1"]["L_c"] == 16 and d["K1"]["own_fwd"] == 0
    assert d["K1"]["n_r"] == 52
    assert d["K2"]["l0"] == 18 and d["K2"]["l0_block"] == 0 and d["K2"]["l0_on_block_edge"] == 0
    assert d["K2"]["L_c"] == 22 and d["K2"]["own_fwd"] == 1 and d["K2"]["n_r"] == 53
    assert d["K3"]["l0"] == 8 and d["K3"]["ns"] == 32 and d["K3"]["L_c"] == 10 and d["K3"]["own_fwd"] == 1
    assert d["K4"]["n_r"] == 80 and d["K4"]["zpb"] == 2


LOOP = ["k_scsec SC_AMP", "k_scrow SCR_AMP"]


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
def test_launch_lists(prec, pname):
    c = jc.K1
    T = 3
    with_b0 = scjoint(c, prec, 2, T, c.l0, c.ns, True)["launches"]
    without = scjoint(c, prec, 2, T, c.l0, c.ns, False)["launches"]
    assert without == ["memset beta", "memset phi", "k_scrow SCR_INIT"] + LOOP * T  # today's, launch for launch
    assert with_b0 == ["memset phi", "k_scsec SC_AB", "k_scrow SCR_ABOUT", "k_scstart"] + LOOP * T
    # with tolerances: the wave form's section launches, the same head
    wave = scjoint(c, prec, 2, T, c.l0, c.ns, True, 0.01, 0.05)["launches"]
    assert wave == ["memset phi", "k_scsec SC_AB", "k_scrow SCR_ABOUT", "k_scstart"] + ["k_scsec_wave SC_AMP", "k_scrow SCR_AMP"] * T
    assert scjoint(c, prec, 2, 0, c.l0, c.ns, True)["launches"] == ["memset phi", "k_scsec SC_AB", "k_scrow SCR_ABOUT", "k_scstart"]


def walk(calls, B=4):
    c = jc.K2
    return {i: (w[0], w[1], w[2], tuple(w[3:])) for i, w in
            enumerate(scjoint(c, SA_PREC_F64, B, 2, c.l0, c.ns, False, calls=calls)["walk"])}


def test_the_staged_state_rule():
    w = walk(["run", "reserve", "run", "power", "run", "llr", "stage", "run0", "llr", "run", "run0", "llr", "fetch",
              "onecall", "run", "encode", "run0", "onehot", "run0", "stage", "soft", "run0", "stage0", "run0", "runbig",
              "reserve", "run", "hard"])
    assert w[0][1:3] == (SA_ERR_ARG, "batch larger than the reserved workspace (sa_sc_reserve)")  # run before reserve
    assert w[2][1:3] == (SA_ERR_ARG, "power allocation not staged")
    assert w[4][1:3] == (SA_ERR_ARG, "nothing staged")                                          # run before stage
    assert w[5][1:3] == (SA_ERR_ARG, "no beta staged")
    assert w[6][1] == 0 and w[6][3] == (1, 1, 0, 4)
    assert w[7][1:3] == (SA_ERR_ARG, "SA_FLAG_BETA0: no beta staged") and w[7][3] == w[6][3]  # refused: state untouched
    assert w[8][1] == SA_ERR_ARG
    assert w[9][1] == 0 and w[9][3] == (1, 1, 1, 4)     # a run leaves its estimate
    assert w[10][1] == 0 and w[11][1] == 0 and w[12][1] == 0
    assert w[13][3] == (1, 0, 0, 0)                    # a one-call entry point overwrites the workspace
    assert w[14][1:3] == (SA_ERR_ARG, "nothing staged")
    assert w[15][3] == (1, 1, 0, 4) and w[16][1] == SA_ERR_ARG
    assert w[17][3] == (1, 1, 1, 4) and w[18][1] == 0
    assert w[19][3] == (1, 1, 0, 4) and w[20][3] == (1, 1, 1, 4) and w[21][1] == 0
    assert w[22][3] == (1, 1, 1, 4) and w[23][1] == 0
    assert w[24][1:3] == (SA_ERR_ARG, "batch larger than the reserved workspace (sa_sc_reserve)")
    assert w[25][3] == (1, 1, 1, 4) and w[26][1] == 0  # a reserve that does not grow keeps the stage
    assert w[27][1] == 0


def test_a_growing_reserve_drops_the_stage():
    c = jc.K1
    a = scjoint(c, SA_PREC_F32, 2, 1, c.l0, c.ns, False, calls=["reserve", "power", "stage", "run"])["walk"]
    assert a[-1][1] == 0
    # the stage of 2 codewords does not cover a run of 3 (`runbig` is B + 1 against a workspace of B)
    assert a[2][3:] == [1, 1, 0, 2]


BAD_RANGES = [("l0 negative", -1, 4, SA_ERR_ARG, "l0 must be non-negative"),
              ("ns zero", 0, 0, SA_ERR_ARG, "ns must be at least 1"),
              ("ns negative", 0, -3, SA_ERR_ARG, "ns must be at least 1"),
              ("past L", 20, 48, SA_ERR_ARG, "section range outside [0, L)"),
              ("l0 at L", 64, 1, SA_ERR_ARG, "section range outside [0, L)")]


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("name,l0,ns,status,text", BAD_RANGES, ids=[b[0] for b in BAD_RANGES])
def test_refused_section_ranges(name, l0, ns, status, text, prec, pname):
    d = scjoint(jc.K1, prec, 2, 2, l0, ns, True)
    assert d.get("error") == status and d["message"] == text


def test_every_legal_l0_is_accepted():
    c = jc.K1
    for l0, ns in ((0, c.L), (0, 1), (c.L - 1, 1), (17, 5), (16, 48)):
        assert "error" not in scjoint(c, SA_PREC_F64, 2, 2, l0, ns, True)


def test_other_refusals():
    c = sc_cases.Case("M1", 8, 1, 40, 2, 4, 2.0, 0.5, ())
    d = scjoint(c, SA_PREC_F32, 1, 1, 0, 8, False)
    assert d.get("error") == SA_ERR_UNSUPPORTED and "M < 2" in d["message"]
    d = scjoint(jc.K1, SA_PREC_F32, 1, 1, 16, 48, True, stop_tol=-1.0)
    assert d.get("error") == SA_ERR_ARG and "stop_tol" in d["message"]
    d = scjoint(jc.K1, SA_PREC_F32, 0, 1, 16, 48, True)
    assert d.get("error") == SA_ERR_ARG
    W = jc.K1.W.copy()
    W[0, 0] = -1.0
    bad = sc_cases.Case("W", 64, 16, 260, 2, 4, 4.0, 0.88, ())
    bad.W = W
    d = scjoint(bad, SA_PREC_F64, 1, 1, 16, 48, True)
    assert d.get("error") == SA_ERR_ARG and "W[0,0] is negative" in d["message"]  # a refused layout is reported first


def test_the_sc_and_scwave_modes_print_what_they_printed():
    c = sc_cases.C
    out = run("sc", [c.L, c.M, c.n, SA_PREC_F32, c.R, c.C] + [repr(float(v)) for v in c.W.reshape(-1)])
    assert out == ('{"R": 5, "C": 3, "L": 15, "M": 16, "n": 185, "n_r": 37, "L_c": 5, "gpc": 2, "G": 6, "zpb": 1, "NZ": 5, '
                   '"own_fwd": 1, "w": 256, "nhi": 16, "E": 1, "sec_lds": 1808, "lds_limit": 163840, "max_blocks": 64, '
                   '"groups": [[0, 0, 4], [0, 4, 1], [1, 5, 4], [1, 9, 1], [2, 10, 4], [2, 14, 1]], '
                   '"zparts": [[0, 0, 37], [1, 37, 37], [2, 74, 37], [3, 111, 37], [4, 148, 37]]}\n')
    w = wc.BY_NAME["D"]
    d = w.case
    out = run("scwave", [d.L, d.M, d.n, SA_PREC_F64, d.R, d.C, 8, 40, repr(w.stop_tol), repr(w.freeze_tol), 1] +
              [repr(float(v)) for v in d.W.reshape(-1)])
    assert out == ('{"wave": 1, "instance": "k_scsec_wave<f64, 1>", "E": 1, "stop_tol": 0.01, "freeze_tol": 0.050000000000000003, '
                   '"late_loads": 1, "grid": [16, 8], "block": 256, "sec_lds": 5024, "lds_limit": 163840, "taul_bytes": 1024, '
                   '"live_bytes": 2560, "R": 10, "C": 8, "G": 16, "gpc": 2}\n')
