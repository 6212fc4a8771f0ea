"""The k_secb instance family: a host model of the chooser and the case table
of tests/test_gpu_secb_instances.py (checked on the CPU by
tests/test_secb_cases_host.py).  No GPU import.

k_secb<real, E, CB, W, ZIL> (csrc/sa_secb.hip) is registered in 70 instances
(secb_lds_attrs_t).  `expected_instance` restates the host rules that pick
one: cb_for and the WB8 / WB16 override of shape_for (csrc/sa_shape.h), zil_for, the bank
conditions of ensure_invb, and the kernel's own condition for its sign-split
gather loop.  62 instances can be selected; the eight with E = 16 and 16-byte
rows (binary32 CB = 4, binary64 CB = 2; both W, both ZIL) cannot: their T tile
W * M * CB * s is 256 KB at W = 16 and 128 KB at W = 8, over the 160 KB and
80 KB limits.  The built-in rule (no WB option) never picks W = 8: cb_for(16)
allows the same T bytes per codeword as cb_for(8) and twice the z bytes, so
its CB is never the smaller one.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import amp_oracle as orc

# ---- the chooser, restated ---------------------------------------------------
K_INVB_ZERO_ROWS = 16          # kInvbZeroRows (sa_common.h)
LDS_HALF, LDS_FULL = 80 * 1024, 160 * 1024
K_SPW = 4                      # sections of the one-codeword kernel's LDS image (sec_lds)
SIZE = {"fp32": 4, "fp64": 8}
E_ALL = (1, 2, 4, 8, 16)

Instance = namedtuple("Instance", "E CB W ZIL banked GS nhi")


def e_of(M):
    """Elements per lane: the smallest power of two with 64 E >= M."""
    E = 1
    while 64 * E < M:
        E *= 2
    return E


def w_of(n, M):
    """2^ceil(log2(max(M + 1, n + 1))), the transform length."""
    w = 1
    while w < max(M + 1, n + 1):
        w *= 2
    return w


def _r16(x):
    return (x + 15) // 16 * 16


def cb_for(prec, M, n, W):
    """shape_for's cb_for: (CB, LDS bytes), (0, 0) where nothing fits."""
    s = SIZE[prec]
    cb = 4 if s == 4 else 2
    while cb >= 1 and M <= 1024:
        zb = _r16((n + K_INVB_ZERO_ROWS) * cb * s)
        tb = W * M * cb * s
        need = max(zb, tb) + W * cb * s + (64 * 8 if s == 8 else 0)
        if need <= (LDS_FULL if (cb == 1 or W > 8) else LDS_HALF):
            return cb, need
        cb >>= 1
    return 0, 0


def _big(prec, M, n):
    """shape_for's `big`: z past the one-codeword kernel's LDS image (no batched kernel)."""
    s = SIZE[prec]
    return n >= 65535 or _r16((n + 1) * s) + K_SPW * M * s + K_SPW * s > LDS_FULL


def expected_instance(prec, L, M, n, B, plan=()):
    """The k_secb instance a decode of B codewords runs on a Hadamard operator
    (L, M, n) of a power-of-two M created with the `plan` options, as
    (E, CB, W, ZIL, banked, GS, nhi); None where no batched kernel runs.
    banked: the bank-aware bucket table is built (a.invb); GS: the kernel
    takes its sign-split gather loop."""
    plan = {p.upper() for p in ((plan,) if isinstance(plan, str) else (plan or ()))}
    s = SIZE[prec]
    E = e_of(M)
    nhi = w_of(n, M) // M
    c8, c16 = ((0, 0), (0, 0)) if _big(prec, M, n) else (cb_for(prec, M, n, 8), cb_for(prec, M, n, 16))
    w16 = True if "WB16" in plan else False if "WB8" in plan else c16[0] >= c8[0]
    W = 16 if (w16 and c16[0] > 0) else 8
    CB = c16[0] if W == 16 else c8[0]
    if CB == 0 or B < 4:  # use_batched
        return None
    rows16 = CB * s == 16
    zil = rows16 and "NO_ZIL" not in plan                                       # zil_for
    banked = (rows16 and "NO_BANKS" not in plan and E >= 4 and nhi >= 2
              and n + K_INVB_ZERO_ROWS <= 65535)                                # ensure_invb
    KH = 2 if (s == 8 or E >= 16 or CB >= 4) else 4                             # kSecbKH64 / kSecbKH32 / 4
    half = nhi // 2
    GS = rows16 and E <= 8 and banked and half > 0 and half % KH == 0          # k_secb's sign-split loop
    return Instance(E, CB, W, zil, banked, GS, nhi)


# ---- the case table ----------------------------------------------------------
P, T_FIXED = 2.0, 3
# reduced CB: the first odd n at which the next larger CB stops fitting
N_REDUCED = {("fp32", 8, 2): 5097, ("fp32", 8, 1): 10217, ("fp32", 16, 2): 10209, ("fp32", 16, 1): 20449,
             ("fp64", 8, 1): 5065, ("fp64", 16, 1): 10177}

Case = namedtuple("Case", "prec E CB W ZIL n plan L M B")


def _case(prec, E, CB, W, zil, n, extra=()):
    plan = ("WB8" if W == 8 else "WB16",) + (() if zil or CB * SIZE[prec] != 16 else ("NO_ZIL",)) + tuple(extra)
    return Case(prec, E, CB, W, zil, n, plan, W + 3, 64 * E, 7 if CB > 1 else 5)


def case_id(c):
    tag = ("-zil" if c.ZIL else "-nozil") if c.CB * SIZE[c.prec] == 16 else ""
    nb = "-nobanks" if "NO_BANKS" in c.plan else ""
    return f"{c.prec}-E{c.E}-CB{c.CB}-W{c.W}{tag}-n{c.n}{nb}"


def _main_cases():
    out = []
    for prec in ("fp32", "fp64"):
        cbmax = 16 // SIZE[prec]
        for W in (8, 16):
            for E in (1, 2, 4, 8):
                M = 64 * E
                for n in (2 * M - 3, 8 * M - 3):
                    for zil in (True, False):
                        out.append(_case(prec, E, cbmax, W, zil, n))
            for n in (2045, 8189):
                out.append(_case(prec, 16, cbmax // 2, W, False, n))
            cb = cbmax // 2
            while cb >= 1:
                for E in E_ALL:
                    if not (E == 16 and cb == cbmax // 2):
                        out.append(_case(prec, E, cb, W, False, N_REDUCED[(prec, W, cb)]))
                cb >>= 1
    return out


def _nobanks_cases():
    return [_case(prec, E, 16 // SIZE[prec], W, zil, 8 * 64 * E - 3, ("NO_BANKS",))
            for prec in ("fp32", "fp64") for W in (8, 16) for E in (4, 8) for zil in (True, False)]


CASES = _main_cases()
NOBANKS_CASES = _nobanks_cases()

# early stop inside a chunk: (prec, CB, E, n by W, ZIL)
T_STOP, RHO_EVEN, RHO_ODD = 25, 0.35, 1.0
_STOP_ROWS = [("fp32", 4, 4, {8: 2045, 16: 2045}, True), ("fp32", 2, 16, {8: 8189, 16: 8189}, False),
              ("fp32", 1, 8, {8: 10217, 16: 20449}, False), ("fp64", 2, 4, {8: 2045, 16: 2045}, True),
              ("fp64", 1, 16, {8: 8189, 16: 8189}, False)]
STOP_CASES = [_case(prec, E, CB, W, zil, ns[W]) for prec, CB, E, ns, zil in _STOP_ROWS for W in (8, 16)]

# the eight registered instances no shape selects: (prec, E, CB, W, ZIL)
UNREACHABLE = [(prec, 16, 16 // SIZE[prec], W, zil) for prec in ("fp32", "fp64") for W in (8, 16)
               for zil in (True, False)]


def instance_key(c):
    return (c.prec, c.E, c.CB, c.W, c.ZIL)


# ---- inputs and the oracle's decodes (computed once per shape) -----------------
def flat_power(L):
    return P / L * np.ones(L)


def rate(L, M, n):
    return L * np.log2(M) / n


def sigma_at(L, M, n, rho=1.0):
    """The noise level at which the rate R / rho is the capacity."""
    return float(np.sqrt(P / (2.0 ** (2.0 * rate(L, M, n) / rho) - 1.0)))


@functools.lru_cache(maxsize=None)
def _transforms(L, M, n):
    return orc.sparc_transforms(L, M, n)


@functools.lru_cache(maxsize=None)
def fixed_reference(L, M, n, B):
    """(ys (B, n), refs (B, L*M)): capacity-rate inputs of seeds 50 + i and
    the oracle's estimates after T_FIXED iterations, the early stop off.
    Read-only: shared by every case of the shape."""
    Ab, Az, _ = _transforms(L, M, n)
    Pl = flat_power(L)
    sg = sigma_at(L, M, n)
    ys = np.stack([orc.rep_inputs(L, M, n, Pl, sg, Ab, 50 + i)[1].reshape(-1) for i in range(B)])
    refs = np.stack([orc._amp_core(ys[i].reshape(-1, 1), Pl, L, M, T_FIXED, Ab, Az, None, early_stop=False)[0]
                     .reshape(-1) for i in range(B)])
    ys.setflags(write=False)
    refs.setflags(write=False)
    return ys, refs


# The exact-tau stop index scatters from draw to draw: codeword i of a stop
# case is seed base + i, the base 50 unless the oracle's stop indices at 50 miss
# the condition test_secb_cases_host.py sets (every even codeword stops at
# least 3 iterations before each odd one); then the first of 60, 70, 80 that meets it.
# (19, 256, 2045) meets it at 50, but its codeword 2 is numerically hard for the
# stop itself: tau == last_tau compares neighbours only, and the binary32
# batched decode's tau never repeats (no stop in 80 iterations on the MI355X,
# where the one-codeword decode of the same input stops at 4).  That is a
# property of the exact-equality stop, not of a kernel: the oracle's own loop
# does not stop within its 25 iterations on other draws (seed 112 at this
# shape, seed 124 at (11, 256, 2045)), nor does a binary64 batched decode
# within 80 (seed 60 at (11, 256, 2045)).  Base 60 there.
STOP_SEED_BASE = {(11, 1024, 8189): 60, (19, 512, 20449): 80, (19, 256, 2045): 60}


@functools.lru_cache(maxsize=None)
def _stop_reference7(L, M, n):
    Ab, Az, _ = _transforms(L, M, n)
    Pl = flat_power(L)
    base = STOP_SEED_BASE.get((L, M, n), 50)
    idx, ys, refs, ts, upd = [], [], [], [], []
    for i in range(7):
        sg = sigma_at(L, M, n, RHO_EVEN if i % 2 == 0 else RHO_ODD)
        ix, y = orc.rep_inputs(L, M, n, Pl, sg, Ab, base + i)
        b, t = orc.amp_test(y, 0, Pl, L, M, T_STOP, Ab, Az)
        # amp_test returns T - 1 both for a stop at T - 1 (T - 1 updates) and
        # for a loop that ran out (T updates): one more iteration tells them apart
        u = t
        if t == T_STOP - 1 and orc.amp_test(y, 0, Pl, L, M, T_STOP + 1, Ab, Az)[1] != t:
            u = T_STOP
        idx.append(ix); ys.append(y.reshape(-1)); refs.append(b.reshape(-1)); ts.append(t); upd.append(u)
    out = (np.stack(idx), np.stack(ys), np.stack(refs), np.asarray(ts), np.asarray(upd))
    for a in out:
        a.setflags(write=False)
    return out


def stop_reference(L, M, n, B):
    """(idx (B, L), ys (B, n), refs (B, L*M), t_ref (B,), updates (B,)):
    codeword i drawn at the capacity noise of rate R / rho (rho = RHO_EVEN for
    even i, RHO_ODD for odd i), the oracle's amp_test with T_STOP iterations,
    and the number of updates behind its estimate.  Read-only."""
    return tuple(a[:B] for a in _stop_reference7(L, M, n))
