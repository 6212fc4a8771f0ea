"""The one-codeword section kernels k_sec, k_secg, k_sec2, k_sec4, k_sec43 and
k_sec44 (csrc/sa_sec.hip): the case table of tests/test_gpu_sec_instances.py,
checked on the CPU by tests/test_sec_cases_host.py.  No GPU import.

The family is registered in 58 instances (sec_lds_attrs_t), 29 per precision.
The chooser is not restated here: every row of the table carries the literal
plan that csrc/sa_shape.h gives the shape on 256 CUs, and the host test
compares each row with the rules themselves (sa_host_check shape).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import amp_oracle as orc
from secb_cases import P, T_FIXED, flat_power, sigma_at

N_CUS = 256
T_START, T_STOP = 2, 25  # the beta0 start's iterations; the oracle loop's own length

Case = namedtuple("Case", "prec L M n B plan sec targ row rs partials gpu")

MULTIWAVE = ("k_sec2", "k_sec4", "k_sec43", "k_sec44")
# template arguments registered per kernel and precision (sec_lds_attrs_t)
REGISTERED = {"k_sec": (1, 2, 4, 8, 16, 32, 64), "k_secg": (1, 2, 4, 8, 16, 32, 64), "k_sec2": (1, 2, 4, 8, 16, 32),
              "k_sec4": (1, 2, 4, 8, 16), "k_sec43": (1, 2), "k_sec44": (1, 2)}


def template_argument(sec, M):
    """The template argument launch_sec / launch_sec2 switch to at a section of
    M columns (M the padded size): E of k_sec / k_secg, M / 128 of k_sec2,
    M / 256 of k_sec4 / k_sec43 / k_sec44."""
    if sec in ("k_sec", "k_secg"):
        E = 1
        while 64 * E < M:
            E *= 2
        return E
    return M // (128 if sec == "k_sec2" else 256)


def _rows(prec, rows, gpu=True):
    return [Case(prec, L, M, n, B, tuple(plan), sec, targ, row, rs, G, gpu) for L, M, n, B, plan, sec, targ, row, rs, G in rows]


# (L, M, n, B, plan, section kernel, template argument, row kernel, row splits, partials)
# n = 2M - 3: w = 2M, nhi = 2.  The first n at which k_secg takes over
# (sec_lds_need(M, n, s, true) > 160 KB) is even; the k_secg rows take the
# odd n after it.
_FP32 = [
    # k_sec4<E4>: 129 pairs, the last with one section; B = 2 and 3 through grid.y
    (257, 256, 509, 1, (), "k_sec4", 1, "k_row2_16", 1, 129),
    (257, 512, 1021, 1, (), "k_sec4", 2, "k_row2_16", 1, 129),
    (257, 1024, 2045, 1, (), "k_sec4", 4, "k_row2_16", 1, 129),
    (257, 2048, 4093, 1, (), "k_sec4", 8, "k_row2_16", 1, 129),
    (257, 4096, 8189, 1, (), "k_sec4", 16, "k_row2", 1, 129),
    (129, 1024, 2045, 2, (), "k_sec4", 4, "k_row2", 1, 65),
    (86, 512, 1021, 3, (), "k_sec4", 2, "k_row2", 1, 43),
    # k_sec2<E2>: M = 128, and the first n of the 16-row window of each larger M
    (257, 128, 253, 1, (), "k_sec2", 1, "k_row2", 1, 129),
    (257, 256, 39904, 1, (), "k_sec2", 2, "k_row2", 1, 129),
    (257, 512, 38880, 1, (), "k_sec2", 4, "k_row2", 1, 129),
    (257, 1024, 36832, 1, (), "k_sec2", 8, "k_row2", 1, 129),
    (257, 2048, 32736, 1, (), "k_sec2", 16, "k_row2", 1, 129),
    (257, 4096, 24544, 1, (), "k_sec2", 32, "k_row2", 1, 129),
    # the window's edges at M = 4096: one row below, its last row, 16 rows on
    (257, 4096, 24543, 1, (), "k_sec4", 16, "k_row2", 1, 129),
    (257, 4096, 24559, 1, (), "k_sec2", 32, "k_row2", 1, 129),
    (257, 4096, 24560, 1, (), "k_sec", 64, "k_row2", 4, 65),
    # k_sec43 (86 triples, the last with two sections) and k_sec44 (65 quads, the last with one)
    (257, 256, 509, 1, ("SEC3",), "k_sec43", 1, "k_row2_16", 1, 86),
    (257, 512, 1021, 1, ("SEC3",), "k_sec43", 2, "k_row2_16", 1, 86),
    (257, 256, 509, 1, ("SEC4Q",), "k_sec44", 1, "k_row2_16", 1, 65),
    (257, 512, 1021, 1, ("SEC4Q",), "k_sec44", 2, "k_row2_16", 1, 65),
    (86, 512, 1021, 3, ("SEC3",), "k_sec43", 2, "k_row2", 1, 29),
    # k_sec<E>: three workgroups, one section in the last, four row splits
    (9, 64, 125, 1, (), "k_sec", 1, "k_row2", 4, 3),
    (9, 128, 253, 1, (), "k_sec", 2, "k_row2", 4, 3),
    (9, 256, 509, 1, (), "k_sec", 4, "k_row2_16", 4, 3),
    (9, 512, 1021, 1, (), "k_sec", 8, "k_row2_16", 4, 3),
    (9, 1024, 2045, 1, (), "k_sec", 16, "k_row2_16", 4, 3),
    (9, 2048, 4093, 1, (), "k_sec", 32, "k_row2_16", 4, 3),
    (9, 4096, 8189, 1, (), "k_sec", 64, "k_row2", 4, 3),
    (9, 48, 125, 1, (), "k_sec", 1, "k_row2", 4, 3),  # a padded section: 16 dead columns
    (1021, 64, 509, 1, (), "k_sec", 1, "k_row2", 1, 256),
    (512, 64, 509, 1, (), "k_sec", 1, "k_row2", 2, 128),
    (343, 64, 509, 1, (), "k_sec", 1, "k_row2", 3, 86),
    (64, 64, 509, 1, (), "k_sec", 1, "k_row2", 4, 16),
    (343, 64, 509, 3, (), "k_sec", 1, "k_row2", 1, 86),
    # k_secg<E>: z in global memory
    (5, 64, 40701, 1, (), "k_secg", 1, "k_row2", 4, 2),
    (5, 128, 40445, 1, (), "k_secg", 2, "k_row2", 4, 2),
    (5, 256, 39933, 1, (), "k_secg", 4, "k_row2", 4, 2),
    (5, 512, 38909, 1, (), "k_secg", 8, "k_row2", 4, 2),
    (5, 1024, 36861, 1, (), "k_secg", 16, "k_row2", 4, 2),
    (5, 2048, 32769, 1, (), "k_secg", 32, "k_row2", 4, 2),  # moved from 32765: K_SECG_MOVED
    (5, 4096, 24573, 1, (), "k_secg", 64, "k_row2", 4, 2),
    (5, 64, 65537, 1, (), "k_secg", 1, "k_row", 4, 2),  # big through the 32-bit rows alone
]
_FP32_HOST = [  # the M <= 512 rule of the triple and quad kernels
    (257, 1024, 2045, 1, ("SEC3",), "k_sec4", 4, "k_row2_16", 1, 129),
    (257, 1024, 2045, 1, ("SEC4Q",), "k_sec4", 4, "k_row2_16", 1, 129),
]
_FP64 = [
    (257, 256, 509, 1, (), "k_sec4", 1, "k_row2", 1, 129),
    (257, 512, 1021, 1, (), "k_sec4", 2, "k_row2", 1, 129),
    (257, 1024, 2045, 1, (), "k_sec4", 4, "k_row2", 1, 129),
    (257, 2048, 4093, 1, (), "k_sec4", 8, "k_row2", 1, 129),
    (257, 4096, 4061, 1, (), "k_sec4", 16, "k_row2", 1, 129),  # sec4_need fits up to n = 4063
    (129, 1024, 2045, 2, (), "k_sec4", 4, "k_row2", 1, 65),
    (86, 512, 1021, 3, (), "k_sec4", 2, "k_row2", 1, 43),
    (257, 128, 253, 1, (), "k_sec2", 1, "k_row2", 1, 129),
    (257, 256, 19424, 1, (), "k_sec2", 2, "k_row2", 1, 129),
    (257, 512, 18400, 1, (), "k_sec2", 4, "k_row2", 1, 129),
    (257, 1024, 16352, 1, (), "k_sec2", 8, "k_row2", 1, 129),
    (257, 2048, 12256, 1, (), "k_sec2", 16, "k_row2", 1, 129),
    (257, 4096, 4064, 1, (), "k_sec2", 32, "k_row2", 1, 129),
    # M = 4096: all four kernels within 30 rows
    (257, 4096, 4063, 1, (), "k_sec4", 16, "k_row2", 1, 129),
    (257, 4096, 4079, 1, (), "k_sec2", 32, "k_row2", 1, 129),
    (257, 4096, 4080, 1, (), "k_sec", 64, "k_row2", 4, 65),
    (257, 4096, 4092, 1, (), "k_secg", 64, "k_row2", 4, 65),
    (257, 256, 509, 1, ("SEC3",), "k_sec43", 1, "k_row2", 1, 86),
    (257, 512, 1021, 1, ("SEC3",), "k_sec43", 2, "k_row2", 1, 86),
    (257, 256, 509, 1, ("SEC4Q",), "k_sec44", 1, "k_row2", 1, 65),
    (257, 512, 1021, 1, ("SEC4Q",), "k_sec44", 2, "k_row2", 1, 65),
    (86, 512, 1021, 3, ("SEC3",), "k_sec43", 2, "k_row2", 1, 29),
    (9, 64, 125, 1, (), "k_sec", 1, "k_row2", 4, 3),
    (9, 128, 253, 1, (), "k_sec", 2, "k_row2", 4, 3),
    (9, 256, 509, 1, (), "k_sec", 4, "k_row2", 4, 3),
    (9, 512, 1021, 1, (), "k_sec", 8, "k_row2", 4, 3),
    (9, 1024, 2045, 1, (), "k_sec", 16, "k_row2", 4, 3),
    (9, 2048, 4093, 1, (), "k_sec", 32, "k_row2", 4, 3),
    (9, 4096, 4080, 1, (), "k_sec", 64, "k_row2", 4, 3),  # (9, 4096, 8189) is k_secg in binary64
    (9, 48, 125, 1, (), "k_sec", 1, "k_row2", 4, 3),
    (1021, 64, 509, 1, (), "k_sec", 1, "k_row2", 1, 256),
    (512, 64, 509, 1, (), "k_sec", 1, "k_row2", 2, 128),
    (343, 64, 509, 1, (), "k_sec", 1, "k_row2", 3, 86),
    (64, 64, 509, 1, (), "k_sec", 1, "k_row2", 4, 16),
    (343, 64, 509, 3, (), "k_sec", 1, "k_row2", 1, 86),
    (5, 64, 20221, 1, (), "k_secg", 1, "k_row2", 4, 2),
    (5, 128, 19965, 1, (), "k_secg", 2, "k_row2", 4, 2),
    (5, 256, 19453, 1, (), "k_secg", 4, "k_row2", 4, 2),
    (5, 512, 18429, 1, (), "k_secg", 8, "k_row2", 4, 2),
    (5, 1024, 16381, 1, (), "k_secg", 16, "k_row2", 4, 2),
    (5, 2048, 12285, 1, (), "k_secg", 32, "k_row2", 4, 2),
    (5, 4096, 4093, 1, (), "k_secg", 64, "k_row2", 4, 2),
    (5, 64, 65537, 1, (), "k_secg", 1, "k_row", 4, 2),
    (129, 4096, 8189, 2, (), "k_secg", 64, "k_row2", 4, 33),  # 33 groups, two codewords
]
_FP64_HOST = [
    (257, 1024, 2045, 1, ("SEC3",), "k_sec4", 4, "k_row2", 1, 129),
    (257, 1024, 2045, 1, ("SEC4Q",), "k_sec4", 4, "k_row2", 1, 129),
]

CASES = _rows("fp32", _FP32) + _rows("fp64", _FP64)
HOST_CASES = _rows("fp32", _FP32_HOST, gpu=False) + _rows("fp64", _FP64_HOST, gpu=False)

# k_secg rows not on the first odd n past the LDS limit: at (5, 2048, 32765) one
# section of five is unsaturated after 3 oracle iterations (share 0.2, under the
# 0.5 the host test asks for); 32769, the next odd n with another transform
# length (w = 65536), has three (0.6)
K_SECG_MOVED = {("fp32", 2048): (32765, 32769)}

# what one codeword runs on the operators of the B > 1 rows (the GPU test compares
# each codeword of the batch with its own one-codeword decode)
ONE_CODEWORD = {
    ("fp32", 129, 1024, 2045, 2, ()): ("k_sec", 16, "k_row2_16", 4, 33),
    ("fp32", 86, 512, 1021, 3, ()): ("k_sec", 8, "k_row2_16", 4, 22),
    ("fp32", 86, 512, 1021, 3, ("SEC3",)): ("k_sec", 8, "k_row2_16", 4, 22),
    ("fp32", 343, 64, 509, 3, ()): ("k_sec", 1, "k_row2", 3, 86),
    ("fp64", 129, 1024, 2045, 2, ()): ("k_sec", 16, "k_row2", 4, 33),
    ("fp64", 86, 512, 1021, 3, ()): ("k_sec", 8, "k_row2", 4, 22),
    ("fp64", 86, 512, 1021, 3, ("SEC3",)): ("k_sec", 8, "k_row2", 4, 22),
    ("fp64", 343, 64, 509, 3, ()): ("k_sec", 1, "k_row2", 3, 86),
    ("fp64", 129, 4096, 8189, 2, ()): ("k_secg", 64, "k_row2", 4, 33),
}

# the first n of the 16-row window in which k_sec2 is selected at M >= 256
# (sec2_need <= 160 KB < sec4_need), by (M, precision)
SEC2_WINDOW = {(256, "fp32"): 39904, (512, "fp32"): 38880, (1024, "fp32"): 36832, (2048, "fp32"): 32736,
               (4096, "fp32"): 24544, (256, "fp64"): 19424, (512, "fp64"): 18400, (1024, "fp64"): 16352,
               (2048, "fp64"): 12256, (4096, "fp64"): 4064}


def case_id(c):
    plan = "".join("-" + p.lower() for p in c.plan)
    return f"{c.prec}-{c.sec}-E{c.targ}-L{c.L}-M{c.M}-n{c.n}-B{c.B}{plan}"


def instance_key(c):
    return (c.sec, c.targ, c.prec)


def shape_of(c):
    return (c.L, c.M, c.n)


# ---- the oracle's transforms without the butterflies that feed nothing ---------
def _fht_rows(x):
    """orc.fht_inplace along the last axis of a (rows, N) array: the same
    butterflies in the same order (stride N / 2 down to 1), every row at once."""
    N = x.shape[-1]
    i = N >> 1
    while i:
        v = x.reshape(x.shape[0], N // (2 * i), 2, i)
        a = v[:, :, 0].copy()
        b = v[:, :, 1]
        v[:, :, 0] = a + b
        v[:, :, 1] = a - b
        i >>= 1


@functools.lru_cache(maxsize=4)
def fast_transforms(L, M, n):
    """(Ab, Az, ordering) of orc.sparc_transforms(L, M, n), bit for bit, at a
    fraction of the cost (tests/test_sec_cases_host.py holds the two equal).

    The oracle transforms w values per section and keeps the last M outputs
    (Az), or transforms a vector whose first w - M entries are zero (Ab).  Of a
    butterfly of stride i >= Mp = 2^ceil(log2 M), Az's outputs depend on the
    difference a - b alone, the upper half: the lower half is never formed.
    In Ab the same butterflies see a = 0, so they copy b and -b, exactly: the
    block of high index h holds (-1)^popcount(h) times the Mp-point transform
    of the section, and negation commutes with every later rounding.  The
    operations that remain are the oracle's own, on the same operands, in the
    same order; the sections are summed in the order 0 .. L - 1 as there."""
    ordering = orc.make_ordering(L, M, n)
    w = orc._w_of(n, M)
    Mp = 1
    while Mp < M:
        Mp *= 2
    o = ordering.astype(np.int64)
    lo = o & (Mp - 1)
    par = o >> int(np.log2(Mp))
    for sh in (16, 8, 4, 2, 1):
        par ^= par >> sh
    sign = np.where(par & 1, -1.0, 1.0)
    rt = np.sqrt(n)
    step = max(1, (1 << 22) // w)  # sections per pass: 32 MB of binary64

    def Ab(b):
        x = np.zeros((L, Mp))
        x[:, Mp - M:] = np.asarray(b, dtype=np.float64).reshape(L, M)
        _fht_rows(x)
        out = np.zeros(n)
        for l in range(L):
            out += sign[l] * x[l, lo[l]]
        return out.reshape(-1, 1) / rt

    def Az(z):
        z = np.asarray(z, dtype=np.float64).reshape(-1)
        out = np.empty((L, M))
        for l0 in range(0, L, step):
            l1 = min(L, l0 + step)
            x = np.zeros((l1 - l0, w))
            np.put_along_axis(x, o[l0:l1], np.broadcast_to(z, (l1 - l0, n)), axis=1)
            while x.shape[1] > Mp:
                h = x.shape[1] // 2
                x = x[:, :h] - x[:, h:]
            _fht_rows(x)
            out[l0:l1] = x[:, Mp - M:]
        return out.reshape(-1, 1) / rt

    return Ab, Az, ordering


# ---- inputs and the oracle's decodes (computed once per shape) -----------------
@functools.lru_cache(maxsize=None)
def _input(L, M, n, i):
    Ab, _, _ = fast_transforms(L, M, n)
    return orc.rep_inputs(L, M, n, flat_power(L), sigma_at(L, M, n), Ab, 50 + i)[1].reshape(-1)


def inputs(L, M, n, B):
    """ys (B, n): capacity-rate inputs of seeds 50 + i.  Read-only."""
    ys = np.stack([_input(L, M, n, i) for i in range(B)])
    ys.setflags(write=False)
    return ys


@functools.lru_cache(maxsize=16)
def estimate_after(L, M, n, i, k):
    """The oracle's estimate of codeword i after k updates, the early stop off."""
    Ab, Az, _ = fast_transforms(L, M, n)
    b = orc._amp_core(_input(L, M, n, i).reshape(-1, 1), flat_power(L), L, M, k, Ab, Az, None,
                      early_stop=False)[0].reshape(-1)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def fixed_reference(L, M, n, B):
    """(ys (B, n), refs (B, L*M)): the inputs and the oracle's estimates after
    T_FIXED iterations, the early stop off.  Read-only: shared by every case
    of the shape."""
    ys = inputs(L, M, n, B)
    Ab, Az, _ = fast_transforms(L, M, n)
    refs = np.stack([orc._amp_core(ys[i].reshape(-1, 1), flat_power(L), L, M, T_FIXED, Ab, Az, None,
                                   early_stop=False)[0].reshape(-1) for i in range(B)])
    refs.setflags(write=False)
    return ys, refs


def start_beta0(L, M, B):
    """beta0 (B, L*M): one column per section at amplitude 1, a different one
    per section and codeword."""
    b0 = np.zeros((B, L, M))
    for i in range(B):
        b0[i, np.arange(L), (7 * np.arange(L) + 3 + 11 * i) % M] = 1.0
    return b0.reshape(B, L * M)


@functools.lru_cache(maxsize=None)
def start_reference(L, M, n, B):
    """refs (B, L*M): orc._amp_core from start_beta0 after T_START iterations, the early stop off."""
    ys = inputs(L, M, n, B)
    Ab, Az, _ = fast_transforms(L, M, n)
    b0 = start_beta0(L, M, B)
    refs = np.stack([orc._amp_core(ys[i].reshape(-1, 1), flat_power(L), L, M, T_START, Ab, Az, b0[i],
                                   early_stop=False)[0].reshape(-1) for i in range(B)])
    refs.setflags(write=False)
    return refs


@functools.lru_cache(maxsize=None)
def product_reference(L, M, n, B):
    """(b (B, L*M), z (B, n), Ab b (B, n), Az z (B, L*M)): random normal
    vectors and the oracle's products.  Read-only."""
    Ab, Az, _ = fast_transforms(L, M, n)
    rs = np.random.RandomState(L * 1000 + M + n)
    b, z = rs.randn(B, L * M), rs.randn(B, n)
    out = (b, z, np.stack([Ab(b[i]).reshape(-1) for i in range(B)]), np.stack([Az(z[i]).reshape(-1) for i in range(B)]))
    for a in out:
        a.setflags(write=False)
    return out
