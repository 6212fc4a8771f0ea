"""CPU: the host rules of coupled state evolution (csrc/sa_scse.h) through the
stand-alone checker `sa_host_check scse`: the class table, the tau slots and the
offsets of every case of tests/sc_se_cases.py against a few lines of Python
that restate the rule, phi^0 and tau^2^0 against the statement, and every
refusal of sa_sc_se's plan with its status."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sc_se_cases as scc
import sc_se_ref
from sparc_ldpc_amd._lib import SA_ERR_ARG, SA_ERR_UNSUPPORTED, SA_SC_MAX_BLOCKS, SA_SE_MAX_M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")


def scse(L, M, T, S, configs):
    """configs: [(n, W, sigma, Pl)].  -> the checker's JSON object."""
    args = [str(v) for v in (len(configs), L, M, T, S)]
    for n, W, sigma, Pl in configs:
        W = np.asarray(W, dtype=np.float64)
        args += [str(n), str(W.shape[0]), str(W.shape[1]), repr(float(sigma))]
        args += [repr(float(v)) for v in W.reshape(-1)] + [repr(float(v)) for v in np.asarray(Pl).reshape(-1)]
    p = subprocess.run([CHECKER, "scse"] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


def _bits(v):
    return struct.pack("<d", float(v))


def classes_of(L, configs):
    """The rule restated: per configuration and column block, the distinct
    powers (bit for bit) in order of first appearance."""
    classes, sec_cls, blk_off, cfg_off, slot_off = [], [], [0], [0], [0]
    for n, W, sigma, Pl in configs:
        C = np.asarray(W).shape[1]
        Lc = L // C
        for c in range(C):
            blk = list(Pl[c * Lc:(c + 1) * Lc])
            Pc = 0.0
            for v in blk:
                Pc += v
            first = {}
            for v in blk:
                if _bits(v) not in first:
                    first[_bits(v)] = len(classes)
                    mult = sum(_bits(u) == _bits(v) for u in blk)
                    classes.append((slot_off[-1] + c, float(np.sqrt(n * v)), mult * v / Pc, mult))
                sec_cls.append(first[_bits(v)])
            blk_off.append(len(classes))
        cfg_off.append(len(classes))
        slot_off.append(slot_off[-1] + C)
    return classes, sec_cls, blk_off, cfg_off, slot_off


@pytest.mark.parametrize("name", list(scc.CASES))
def test_plan(name):
    c = scc.case(name)
    configs = [(c.n[b], c.W[b], c.sigma[b], c.Pl[b]) for b in range(c.B)]
    d = scse(c.L, c.M, c.T, c.S, configs)
    assert "error" not in d, d
    classes, sec_cls, blk_off, cfg_off, slot_off = classes_of(c.L, configs)
    assert d["K"] == len(classes) and d["NS"] == sum(c.C) and d["NR"] == sum(c.R)
    assert (d["Rmax"], d["Cmax"]) == (max(c.R), max(c.C))
    assert d["slot_off"] == slot_off and d["blk_off"] == blk_off and d["cfg_off"] == cfg_off
    assert d["row_off"] == [0] + list(np.cumsum(c.R))
    assert d["w_off"] == [0] + list(np.cumsum([r * k for r, k in zip(c.R, c.C)]))
    assert d["sec_cls"] == sec_cls
    assert len(d["classes"]) == len(classes)
    for got, want in zip(d["classes"], classes):
        assert got[0] == want[0] and got[3] == want[3]
        assert got[1] == want[1] and got[2] == want[2], (got, want)  # c and the weight: the same bits
    # every class reads its own (configuration, column block) slot, also where two blocks hold one power
    for b in range(c.B):
        for l in range(c.L):
            assert d["classes"][sec_cls[b * c.L + l]][0] == slot_off[b] + l // (c.L // c.C[b])
    # the chunking
    SC = min(16, 4096 // c.M)
    assert d["SC"] == SC and d["NCH"] == -(-c.S // SC) and d["grid"] == d["NCH"] * -(-d["K"] // d["classes_per_group"])
    assert d["classes_per_group"] == 8 and d["max_blocks"] == SA_SC_MAX_BLOCKS and d["max_M"] == SA_SE_MAX_M
    # P_c, sigma^2, phi^0 and tau^2^0 are the statement's, bit for bit
    for b in range(c.B):
        Pc = sc_se_ref.block_powers(c.Pl[b], c.C[b])
        assert d["Pc"][slot_off[b]:slot_off[b + 1]] == Pc.tolist()
        assert d["sig2"][b] == c.sigma[b] * c.sigma[b]
        assert d["phi0"][d["row_off"][b]:d["row_off"][b + 1]] == c.phi[b][0].tolist()
        assert d["tau20"][slot_off[b]:slot_off[b + 1]] == c.tau2[b][0].tolist()


def test_flat_tail_across_blocks_is_two_classes():
    c = scc.case("pa_blocks")
    d = scse(c.L, c.M, c.T, c.S, [(c.n[0], c.W[0], c.sigma[0], c.Pl[0])])
    Lc = c.L // c.C[0]
    assert c.Pl[0][2 * Lc] == c.Pl[0][3 * Lc]  # one power's bits in the last two blocks
    k2, k3 = d["sec_cls"][2 * Lc], d["sec_cls"][3 * Lc]
    assert k2 != k3 and d["classes"][k2][0] == 2 and d["classes"][k3][0] == 3
    assert d["classes"][k2][3] == Lc and d["classes"][k3][3] == Lc
    assert d["blk_off"] == [0, Lc, 2 * Lc, 2 * Lc + 1, 2 * Lc + 2]


def _refusals():
    c = scc.case("band_2_4")
    L, M, T, S = c.L, c.M, c.T, c.S
    n, W, sg, Pl = c.n[0], c.W[0], c.sigma[0], c.Pl[0]
    ok = (n, W, sg, Pl)
    big = SA_SC_MAX_BLOCKS + 1
    bad = {}

    def one(name, status, text, L=L, M=M, T=T, S=S, cfg=ok, first=None):
        bad[name] = (L, M, T, S, ([first] if first else []) + [cfg], status, text)

    one("R does not divide n", SA_ERR_ARG, "does not divide n = 161", cfg=(161, W, sg, Pl))
    one("C does not divide L", SA_ERR_ARG, "does not divide L = 30", L=30, cfg=(n, W, sg, Pl[:30]))
    for name, at, v, text in (("negative entry", (1, 0), -0.5, "W[1,0] is negative"), ("nan entry", (2, 1), np.nan, "W[2,1] is not finite"),
                              ("inf entry", (2, 2), np.inf, "W[2,2] is not finite")):
        w = W.copy(); w[at] = v
        one(name, SA_ERR_ARG, text, cfg=(n, w, sg, Pl))
    w = W.copy(); w[4, :] = 0
    one("zero row", SA_ERR_ARG, "W row 4", cfg=(n, w, sg, Pl))
    w = W.copy(); w[:, 1] = 0
    one("zero column", SA_ERR_ARG, "W column 1", cfg=(n, w, sg, Pl))
    one("R above the limit", SA_ERR_UNSUPPORTED, "R above SA_SC_MAX_BLOCKS", L=4, cfg=(big * 2, np.ones((big, 1)), sg, np.ones(4)))
    one("C above the limit", SA_ERR_UNSUPPORTED, "C above SA_SC_MAX_BLOCKS", L=big, cfg=(128, np.ones((1, big)), sg, np.ones(big)))
    one("M below 2", SA_ERR_ARG, "M < 2", M=1)
    one("M above the limit", SA_ERR_UNSUPPORTED, "M above SA_SE_MAX_M", M=SA_SE_MAX_M + 1)
    for name, v in (("sigma zero", 0.0), ("sigma negative", -0.5), ("sigma inf", np.inf), ("sigma nan", np.nan)):
        one(name, SA_ERR_ARG, "sigma[0] must be finite and > 0", cfg=(n, W, v, Pl))
    p = Pl.copy(); p[3] = -0.1
    one("negative power", SA_ERR_ARG, "Pl[0][3] must be finite and >= 0", cfg=(n, W, sg, p))
    p = Pl.copy(); p[5] = np.inf
    one("infinite power", SA_ERR_ARG, "Pl[0][5] must be finite and >= 0", cfg=(n, W, sg, p))
    p = Pl.copy(); p[8:16] = 0
    one("a block without power", SA_ERR_ARG, "P_c = 0 for column block 1", cfg=(n, W, sg, p))
    one("T below 1", SA_ERR_ARG, "T < 1", T=0)
    one("S below 1", SA_ERR_ARG, "S < 1", S=0)
    one("S above the limit", SA_ERR_UNSUPPORTED, "S above 2^24", S=(1 << 24) + 1)
    # the message names the configuration
    one("the second configuration", SA_ERR_ARG, "configuration 1: R = 5 does not divide n = 161", cfg=(161, W, sg, Pl), first=ok)
    return bad


REFUSALS = _refusals()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(name):
    L, M, T, S, configs, status, text = REFUSALS[name]
    d = scse(L, M, T, S, configs)
    assert d.get("error") == status, d
    assert text in d["message"], d


def test_m_need_not_be_a_power_of_two():
    c = scc.case("band_2_4")
    assert "error" not in scse(c.L, 48, c.T, c.S, [(c.n[0], c.W[0], c.sigma[0], c.Pl[0])])
    assert "error" not in scse(c.L, SA_SE_MAX_M, c.T, c.S, [(c.n[0], c.W[0], c.sigma[0], c.Pl[0])])
