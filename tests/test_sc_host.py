"""CPU: the host rules of the spatially coupled decoder (csrc/sa_sc.h) through
the stand-alone checker `sa_host_check sc`: the section-group and z^2-partial
layout of cases A-D, re-derived here from what the checker prints, and every
refusal of sa_sc_create with its status."""
import json
import os
import subprocess

import numpy as np
import pytest

import sc_cases
from sparc_ldpc_amd._lib import SA_ERR_ARG, SA_ERR_UNSUPPORTED, SA_PREC_F32, SA_PREC_F64, SA_SC_MAX_BLOCKS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
LDS_BYTES = 160 * 1024  # a CU's LDS on gfx950


def sc(L, M, n, prec, W):
    W = np.asarray(W, dtype=np.float64)
    R, C = W.shape
    p = subprocess.run([CHECKER, "sc"] + [str(v) for v in (L, M, n, prec, R, C)] + [repr(float(v)) for v in W.reshape(-1)],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


@pytest.mark.parametrize("prec", [SA_PREC_F32, SA_PREC_F64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", sc_cases.LAYOUT_CASES, ids=lambda c: c.name)
def test_layout(case, prec):
    d = sc(case.L, case.M, case.n, prec, case.W)
    assert "error" not in d, d
    R, C, L, n = case.R, case.C, case.L, case.n
    assert (d["R"], d["C"], d["n_r"], d["L_c"]) == (R, C, n // R, L // C)
    assert d["max_blocks"] == SA_SC_MAX_BLOCKS
    # every section in exactly one group, no group across a column block
    count = np.zeros(L, dtype=int)
    assert len(d["groups"]) == d["G"] == C * -(-d["L_c"] // 4)
    for c, l0, cnt in d["groups"]:
        assert 1 <= cnt <= 4
        assert l0 // d["L_c"] == c and (l0 + cnt - 1) // d["L_c"] == c
        count[l0:l0 + cnt] += 1
    assert (count == 1).all()
    assert d["own_fwd"] == int(d["L_c"] % 4 != 0)
    # every row in exactly one z^2 partial, none across a row block
    rows = np.zeros(n, dtype=int)
    assert len(d["zparts"]) == d["NZ"] == R * -(-d["n_r"] // 64)
    for r, i0, cnt in d["zparts"]:
        assert 1 <= cnt <= 64
        assert i0 // d["n_r"] == r and (i0 + cnt - 1) // d["n_r"] == r
        rows[i0:i0 + cnt] += 1
    assert (rows == 1).all()
    # the LDS image: z slots, 4 sections' T, the block arrays; within the CU's
    s = 4 if prec == SA_PREC_F32 else 8
    zb = -(-(n + 1) * s // 16) * 16
    assert d["sec_lds"] == zb + 4 * case.M * s + 4 * s + 3 * SA_SC_MAX_BLOCKS * s + 16
    assert d["sec_lds"] <= d["lds_limit"] == LDS_BYTES


def _refusals():
    A = sc_cases.A
    W = A.W
    bad = {}
    bad["R does not divide n"] = (A.L, A.M, 161, W, SA_ERR_ARG, "does not divide n")
    bad["C does not divide L"] = (30, A.M, A.n, W, SA_ERR_ARG, "does not divide L")
    w = W.copy(); w[1, 0] = -0.5
    bad["negative entry"] = (A.L, A.M, A.n, w, SA_ERR_ARG, "W[1,0] is negative")
    w = W.copy(); w[2, 1] = np.nan
    bad["nan entry"] = (A.L, A.M, A.n, w, SA_ERR_ARG, "W[2,1] is not finite")
    w = W.copy(); w[2, 2] = np.inf
    bad["inf entry"] = (A.L, A.M, A.n, w, SA_ERR_ARG, "W[2,2] is not finite")
    w = W.copy(); w[4, :] = 0
    bad["zero row"] = (A.L, A.M, A.n, w, SA_ERR_ARG, "W row 4")
    w = W.copy(); w[:, 1] = 0
    bad["zero column"] = (A.L, A.M, A.n, w, SA_ERR_ARG, "W column 1")
    big = SA_SC_MAX_BLOCKS + 1
    bad["R above the limit"] = (4, 64, big * 2, np.ones((big, 1)), SA_ERR_UNSUPPORTED, "R above SA_SC_MAX_BLOCKS")
    bad["C above the limit"] = (big, 64, 128, np.ones((1, big)), SA_ERR_UNSUPPORTED, "C above SA_SC_MAX_BLOCKS")
    bad["M not a power of two"] = (A.L, 48, A.n, W, SA_ERR_UNSUPPORTED, "M must be a power of two")
    return bad


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    L, M, n, W, status, text = REFUSALS[name]
    d = sc(L, M, n, SA_PREC_F32, W)
    assert d.get("error") == status, d
    assert text in d["message"]


def test_z_past_the_lds_image_is_unsupported():
    # binary64: 8 (n + 1) + 4 M 8 past 160 KB
    d = sc(64, 64, 21000, SA_PREC_F64, np.ones((1, 1)))
    assert d.get("error") == SA_ERR_UNSUPPORTED and "n too large" in d["message"]
    assert "error" not in sc(64, 64, 21000, SA_PREC_F32, np.ones((1, 1)))
