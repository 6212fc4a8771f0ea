"""CPU checks of the launch sequence of an AMP decode (csrc/sa_seq.h:
decode_seq, for_each_step) through the stand-alone checker
sparc_ldpc_amd/sa_host_check seq: which launches a decode of (shape, B, T,
flags, beta0) makes, which buffer each section step reads and writes, and what
is left pending.  Every expected list is written here by hand from the rule
(DESIGN.md section 2), on 256 CUs; nothing is computed by a second call of the
code under test."""
import json
import os
import subprocess
from collections import Counter

import pytest

import sec_cases
import secb_cases
from sparc_ldpc_amd._lib import (SA_BACKEND_DENSE, SA_BACKEND_HADAMARD, SA_FLAG_NO_EARLY_STOP, SA_PREC_F32, SA_PREC_F64,
                                 plan_bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
PREC = {"fp32": SA_PREC_F32, "fp64": SA_PREC_F64}
N_CUS = 256
ROW_INIT0, ROW_INIT, ROW_AMP = 0, 1, 2


def seq(prec, L, M, n, B, T, *, stop, b0, plan=(), profiled=False, backend=SA_BACKEND_HADAMARD):
    flags = 0 if stop else SA_FLAG_NO_EARLY_STOP
    p = subprocess.run([CHECKER, "seq"] + [str(int(a)) for a in (L, M, n, backend, PREC[prec], plan_bits(plan), N_CUS, B, T,
                                                                  flags, b0, profiled)],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    d = json.loads(p.stdout)
    if "error" not in d:
        assert d["nsteps"] == len(d["steps"]), d  # the closed-form count is the walk's
    return d


# ---- the steps, as the checker prints them -----------------------------------
def _step(kind, **kw):
    s = dict(kind=kind, t=0, mode=0, rd=0, wr=0, bzero=0, decide=0, itset=0, G=0, Gb=0, es=0)
    s.update(kw)
    return s


def row(mode, G, Gb=None, t=0, es=0, itset=0):
    return _step("row", mode=mode, G=G, Gb=G if Gb is None else Gb, t=t, es=es, itset=itset)


def kinds(d):
    return [s["kind"] for s in d["steps"]]


def sides(d):
    return [(s["rd"], s["wr"]) for s in d["steps"] if s["kind"] in ("sec", "sec_mw")]


# ---- c2, the headline ----------------------------------------------------------
C2 = ("fp32", 512, 512, 4608, 1, 64)  # 256 pairs on 256 CUs: k_sec4 + k_row2, G = Gb = 256


def _c2_loop(es, bzero0, flip=0, G=256):
    """[section t, row t] for t = 0 .. 63, no iters write, nothing fused."""
    out = []
    for t in range(64):
        rd = (t ^ flip) & 1
        out.append(_step("sec_mw", t=t, rd=rd, wr=1 - rd, es=es, bzero=int(bzero0 and t == 0)))
        out.append(row(ROW_AMP, G, t=t, es=es))
    return out


def test_c2_headline_is_128_launches_and_a_deferred_row():
    d = seq(*C2, stop=False, b0=False)
    want = [row(ROW_INIT0, 256, itset=-1)] + _c2_loop(0, True)[:-1]
    want[-1].update(decide=1, itset=64)
    assert want[1]["rd"] == 0 and want[-1] == _step("sec_mw", t=63, rd=1, wr=0, decide=1, itset=64)  # T even: flip = 0
    assert d["steps"] == want
    assert len(d["steps"]) == 128 and Counter(kinds(d)) == {"row": 64, "sec_mw": 64}
    assert (d["fused"], d["zil"], d["beta_final"]) == (1, 0, 0)
    assert d["row"] == row(ROW_AMP, 256, t=63, es=0, itset=0)


def test_c2_without_the_fused_tail_is_129_launches():
    d = seq(*C2, stop=False, b0=False, plan=("NO_FUSED_TAIL",))
    want = [row(ROW_INIT0, 256, itset=-1)] + _c2_loop(0, True)
    want[-1]["itset"] = 64  # the last row step sets iters
    assert d["steps"] == want and len(want) == 129  # (and k_decide: DESIGN.md section 8 counts 130 -> 128)
    assert (d["fused"], d["row"], d["beta_final"]) == (0, None, 0)


def test_c2_with_the_early_stop_keeps_beta_final():
    d = seq(*C2, stop=True, b0=False)
    want = [row(ROW_INIT0, 256, itset=-1)] + _c2_loop(1, True)
    want[-1]["itset"] = 64
    want.append(_step("beta_final"))
    assert d["steps"] == want
    assert (d["fused"], d["row"], d["beta_final"]) == (0, None, 1)


def test_c2_from_beta0():
    d = seq(*C2, stop=False, b0=True)
    # A beta0 by k_sec: Shape::G = 128 groups of four sections; no bzero; beta0 lies in d_beta: flip = 0
    want = [_step("sec_ab"), row(ROW_INIT, 128, itset=-1)] + _c2_loop(0, False)[:-1]
    want[-1].update(decide=1, itset=64)
    assert d["steps"] == want and len(want) == 129
    assert (d["fused"], d["beta_final"]) == (1, 0) and d["row"] == row(ROW_AMP, 256, t=63)


def test_c2_profiled_has_no_fused_tail():
    d = seq(*C2, stop=False, b0=False, profiled=True)
    want = [row(ROW_INIT0, 256, itset=-1)] + _c2_loop(0, True)
    want[-1]["itset"] = 64
    assert d["steps"] == want and (d["fused"], d["row"]) == (0, None)


# ---- T parity at the smallest pair shape ------------------------------------------
# (T, stop, beta0): the sides (read, written; 0 = d_beta, 1 = d_beta2) of the
# section steps, and whether k_beta_final runs.  With the stop off and no beta0
# the ping-pong starts on the side that ends in d_beta.
PARITY = {
    (1, True, False): ([(0, 1)], 1), (2, True, False): ([(0, 1), (1, 0)], 1),
    (3, True, False): ([(0, 1), (1, 0), (0, 1)], 1),
    (1, True, True): ([(0, 1)], 1), (2, True, True): ([(0, 1), (1, 0)], 1),
    (3, True, True): ([(0, 1), (1, 0), (0, 1)], 1),
    (1, False, True): ([(0, 1)], 1), (2, False, True): ([(0, 1), (1, 0)], 0),
    (3, False, True): ([(0, 1), (1, 0), (0, 1)], 1),
    (1, False, False): ([(1, 0)], 0), (2, False, False): ([(0, 1), (1, 0)], 0),
    (3, False, False): ([(1, 0), (0, 1), (1, 0)], 0),
}


@pytest.mark.parametrize("plan,G", [((), 129), (("SEC3",), 86), (("SEC4Q",), 65)], ids=["pairs", "triples", "quads"])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_parity_of_the_pair_triple_and_quad_kernels(prec, plan, G):
    for (T, stop, b0), (want_sides, bf) in PARITY.items():
        d = seq(prec, 257, 256, 509, 1, T, stop=stop, b0=b0, plan=plan)
        assert sides(d) == want_sides and d["beta_final"] == bf, (T, stop, b0, d)
        fused = int(not stop)
        start = ["sec_ab", "row"] if b0 else ["row"]  # no zero fill: the first launch takes zero
        loop = ["sec_mw", "row"] * T
        assert kinds(d) == start + (loop[:-1] if fused else loop) + ["beta_final"] * bf, (T, stop, b0)
        sec = [s for s in d["steps"] if s["kind"] == "sec_mw"]
        assert [s["bzero"] for s in sec] == [int(not b0)] + [0] * (T - 1)
        assert [(s["decide"], s["itset"]) for s in sec] == [(0, 0)] * (T - 1) + [(fused, T * fused)]
        rows = [s for s in d["steps"] if s["kind"] == "row"]
        assert rows[0] == (row(ROW_INIT, 65, itset=-1) if b0 else row(ROW_INIT0, G, itset=-1))  # ceil(257 / 4) = 65
        assert rows[1:] == [row(ROW_AMP, G, t=t, es=int(stop), itset=T if t == T - 1 else 0) for t in range(T - fused)]
        assert d["fused"] == fused and d["row"] == (row(ROW_AMP, G, t=T - 1) if fused else None)


# k_sec2, k_sec, k_secg: (T, stop) -> beta_final; the ping-pong always starts in d_beta
SIDES3 = [(0, 1), (1, 0), (0, 1)]
PLAIN_BF = {(1, True): 1, (2, True): 1, (3, True): 1, (1, False): 1, (2, False): 0, (3, False): 1}


@pytest.mark.parametrize("shape,kind,G", [((257, 128, 253), "sec_mw", 129), ((9, 64, 125), "sec", 3), ((9, 48, 125), "sec", 3),
                                          ((5, 64, 40701), "sec", 2)], ids=["k_sec2", "k_sec", "padded", "k_secg"])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_the_kernels_that_neither_take_zero_nor_decide(prec, shape, kind, G):
    L, M, n = shape
    G0 = (L + 3) // 4
    for (T, stop), bf in PLAIN_BF.items():
        for b0 in (False, True):
            d = seq(prec, L, M, n, 1, T, stop=stop, b0=b0)
            es = int(stop)
            want = [_step("sec_ab"), row(ROW_INIT, G0, itset=-1)] if b0 else [_step("zero_beta"), row(ROW_INIT0, G, itset=-1)]
            for t in range(T):
                want.append(_step(kind, t=t, rd=SIDES3[t][0], wr=SIDES3[t][1], es=es))
                want.append(row(ROW_AMP, G, t=t, es=es, itset=T if t == T - 1 else 0))
            want += [_step("beta_final")] * bf
            assert d["steps"] == want, (T, stop, b0)
            assert (d["fused"], d["row"], d["zil"], d["beta_final"]) == (0, None, 0, bf)


def test_the_padded_section_has_dead_columns():
    p = subprocess.run([CHECKER, "shape", "9", "48", "125", "0", "0", "0", str(N_CUS), "1"], capture_output=True, text=True)
    assert json.loads(p.stdout)["dead"] == 16


# ---- batched and dense ---------------------------------------------------------------
def _smallest_batched(prec):
    return min((c for c in secb_cases.CASES if c.prec == prec), key=lambda c: (c.L * c.M * c.n, len(c.plan)))


def _zil(prec, L, M, n, B, plan):
    p = subprocess.run([CHECKER, "shape"] + [str(a) for a in (L, M, n, SA_BACKEND_HADAMARD, PREC[prec], plan_bits(plan),
                                                              N_CUS, B)], capture_output=True, text=True)
    return json.loads(p.stdout)["zil"]


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("stop", [True, False], ids=["stop", "fixed"])
@pytest.mark.parametrize("b0", [False, True], ids=["zero", "beta0"])
def test_batched_decodes(prec, stop, b0):
    c = _smallest_batched(prec)
    assert (c.L, c.M, c.n, c.W) == (11, 64, 125, 8)
    es = int(stop)
    # (shape, B, plan, T, Gb = ceil(L / W), Shape::G = ceil(L / 4)): the smallest row, and c4 (W = 16)
    for L, M, n, B, plan, T, Gb, G0 in ((c.L, c.M, c.n, 4, c.plan, 3, 2, 3), (768, 512, 8294, 256, (), 64, 48, 192)):
        d = seq(prec, L, M, n, B, T, stop=stop, b0=b0, plan=plan)
        want = [_step("fill_iters")]
        want += [_step("sec_ab"), row(ROW_INIT, G0)] if b0 else [_step("zero_beta"), row(ROW_INIT0, Gb)]
        for t in range(T):
            want += [_step("sec_b", t=t, es=es), row(ROW_AMP, Gb, t=t, es=es)]
        want.append(_step("iters_final", itset=T))
        assert d["steps"] == want
        assert (d["fused"], d["row"], d["beta_final"]) == (0, None, 0)
        assert d["zil"] == _zil(prec, L, M, n, B, plan) == 1  # 16-byte rows of CB codewords in both precisions


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("b0", [False, True], ids=["zero", "beta0"])
def test_dense_decodes(B, b0):
    # Gd = ceil(32 / 4) = 8 denoiser groups; the A beta partial count is device state (0 here)
    d = seq("fp32", 32, 64, 192, B, 2, stop=True, b0=b0, backend=SA_BACKEND_DENSE)
    want = [_step("fill_iters")] + ([_step("dense_start")] if b0 else [_step("zero_beta"), row(ROW_INIT0, 0, 8)])
    for t in range(2):
        want += [_step("dense_iter", t=t, es=1), row(ROW_AMP, 0, 8, t=t, es=1)]
    want.append(_step("iters_final", itset=2))
    assert d["steps"] == want
    assert (d["fused"], d["row"], d["zil"], d["beta_final"]) == (0, None, 0, 0)


@pytest.mark.parametrize("stop", [True, False], ids=["stop", "fixed"])
def test_no_iterations(stop):
    d = seq("fp32", 257, 256, 509, 1, 0, stop=stop, b0=False)
    assert d["steps"] == [_step("fill_iters"), _step("zero_beta"), row(ROW_INIT0, 129), _step("iters_final")]
    d0 = seq("fp32", 257, 256, 509, 1, 0, stop=stop, b0=True)
    assert d0["steps"] == [_step("fill_iters"), _step("sec_ab"), row(ROW_INIT, 65), _step("iters_final")]
    for x in (d, d0):
        assert (x["fused"], x["row"], x["beta_final"]) == (0, None, 0)


def test_a_refused_shape_is_reported():
    p = subprocess.run([CHECKER, "seq", "4", "8192", "100", "0", "0", "0", str(N_CUS), "1", "3", "0", "0", "0"],
                       capture_output=True, text=True)
    d = json.loads(p.stdout)
    assert p.returncode == 0 and d["error"] == -5 and "M must be <= 4096" in d["message"]


# ---- every shape of the case tables: the counts in closed form -----------------------
def _counts(T, stop, b0, *, it_row, takes_zero, decides, one_codeword, kind):
    """Launches per kind of a decode of T > 0 iterations.  it_row: a k_row2
    decode of the one-codeword kernels (the iters writes ride on row launches);
    takes_zero / decides: the kernel can take the previous estimate as zero /
    end a decode with the stop off (k_sec4, k_sec43, k_sec44 in front of k_row2,
    no padded section)."""
    bz = takes_zero and not b0
    flip = (T & 1) if (bz and not stop) else 0
    ft = decides and not stop
    home = (not stop) and (((T - 1) ^ flip) & 1)
    c = Counter({kind: T, "row": 1 + T - int(ft)})
    c["fill_iters"] = c["iters_final"] = int(not it_row)
    c["sec_ab"] = int(b0)
    c["zero_beta"] = int(not b0 and not bz)
    c["beta_final"] = int(one_codeword and not home)
    return +c


ALL = [(c, "sec") for c in sec_cases.CASES + sec_cases.HOST_CASES] + \
      [(c, "secb") for c in secb_cases.CASES + secb_cases.NOBANKS_CASES + secb_cases.STOP_CASES]


@pytest.mark.parametrize("case,table", ALL, ids=[t + "-" + (sec_cases if t == "sec" else secb_cases).case_id(c) for c, t in ALL])
def test_counts_at_every_case_of_the_tables(case, table):
    c = case
    if table == "sec":
        it_row = c.row in ("k_row2", "k_row2_16")
        zero = c.sec in ("k_sec4", "k_sec43", "k_sec44")
        kw = dict(it_row=it_row, takes_zero=zero, decides=zero and it_row, one_codeword=True,
                  kind="sec_mw" if c.sec in sec_cases.MULTIWAVE else "sec")
        Ts = (sec_cases.T_FIXED, sec_cases.T_START, sec_cases.T_STOP)
    else:
        kw = dict(it_row=False, takes_zero=False, decides=False, one_codeword=False, kind="sec_b")
        Ts = (secb_cases.T_FIXED, secb_cases.T_STOP)
    for T in Ts:
        for stop in (True, False):
            for b0 in (False, True):
                d = seq(c.prec, c.L, c.M, c.n, c.B, T, stop=stop, b0=b0, plan=c.plan)
                want = _counts(T, stop, b0, **kw)
                assert Counter(kinds(d)) == want and d["nsteps"] == sum(want.values()), (T, stop, b0, d)
                assert d["fused"] == int(kw["decides"] and not stop)
