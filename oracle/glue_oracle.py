"""CPU oracle for the SPARC <-> LDPC glue of the joint decoder — TEST
INFRASTRUCTURE ONLY (nothing under ``sparc_ldpc_amd/`` imports it).

Each operation of the glue (encode, cancel, sp2bp + LLR, bp2sp, the rescale
of the sections AMP keeps, hard indices, threshold decisions, one-hot β₀) is
restated from its definition in ``np.longdouble`` — the reference lines are
cited per function — and not from the device kernels: no staging, no
tables, no special cases beyond the ones the reference's own expressions have
(``nan_to_num``, ``app < 0``, ``> threshold``).  Two things stay in binary64
because the reference defines them there: c_l = np.sqrt(n * Pl_l), and the
ordered sum p of ``sp2bp`` whose rounding decides the LLR of a p next to 1
(``sp2bp`` accumulates in the dtype it is given).  Where the platform's
long double is wider than binary64 (x86: 64-bit significand) the oracle's own
rounding is 2^-11 of a binary64 ulp per operation and is negligible against
the bounds the tests set; ``tests/test_glue_oracle.py`` pins the oracle to
fixtures captured from the reference.

Shapes: β (B, L·M), y (B, n), idx (B, ns) int (−1: section not decided),
app / llr (B, ns·log2 M), MSB first within a section.
"""
from __future__ import annotations

import numpy as np

from .amp_oracle import _w_of

LD = np.longdouble
F64_MAX = np.finfo(np.float64).max

__all__ = [
    "LD", "coeffs", "column_signs", "column_sum", "encode", "cancel", "onehot", "sp2bp", "llr_of_p", "llr",
    "bp2sp", "bit_marginals", "soft_sections", "soft_beta0", "rescale", "hard_indices", "threshold_indices",
]


def _ld(a):
    return np.asarray(a, dtype=LD)


def coeffs(n, Pl):
    """c_l = np.sqrt(n * Pl_l), the binary64 number of sparc_ldpc.py:214: the
    non-zero value of a codeword's section and the divisor of :470 are that
    double, a parameter of the code like Pl itself; widened here."""
    return _ld(np.sqrt(n * np.asarray(Pl, dtype=np.float64).reshape(-1)))


def _lgm(M):
    lgm = int(M).bit_length() - 1
    assert M >= 2 and 1 << lgm == M, "the bit-level glue needs M a power of two"
    return lgm


def column_signs(ordering, M, n, sections, idx):
    """±1 (B, ns, n): √n · A[r, l·M + i] for l = sections[j], i = idx[b, j], with
    A[r, l·M + i] = (−1)^popcount(ordering[l, r] & (w − M + i)) / √n
    (amp_oracle.dense_design_matrix; sparc_ldpc.py:65-77).  An idx < 0 gives 0."""
    w = _w_of(n, M)
    idx = np.asarray(idx, dtype=np.int64)
    sections = np.asarray(sections, dtype=np.int64).reshape(-1)
    assert idx.ndim == 2 and idx.shape[1] == sections.size
    assert np.all(idx < M)
    col = (w - M + np.where(idx < 0, 0, idx)).astype(np.uint64)             # (B, ns)
    o = np.asarray(ordering)[sections, :n].astype(np.uint64)                 # (ns, n)
    v = o[None, :, :] & col[:, :, None]
    par = np.zeros(v.shape, dtype=np.uint64)
    while np.any(v):
        par ^= v & np.uint64(1)
        v = v >> np.uint64(1)
    sgn = np.where(par == 1, -1, 1).astype(np.int64)
    return sgn * (idx >= 0)[:, :, None]


def column_sum(ordering, M, n, Pl, idx, sections=None):
    """Σ_j ± c_l / √n over the decided sections -> (B, n) long double, and the
    same sum of magnitudes Σ_j c_l / √n (B,) (the scale of its rounding)."""
    Pl = _ld(Pl).reshape(-1)
    idx = np.asarray(idx, dtype=np.int64)
    if sections is None:
        sections = np.arange(Pl.size)
    sections = np.asarray(sections, dtype=np.int64).reshape(-1)
    c = coeffs(n, Pl)[sections]
    sgn = column_signs(ordering, M, n, sections, idx)
    rt = np.sqrt(LD(n))
    x = (sgn.astype(LD) * c[None, :, None]).sum(axis=1) / rt
    mag = ((idx >= 0).astype(LD) * c[None, :]).sum(axis=1) / rt
    return x, mag


def encode(ordering, M, n, Pl, idx, noise=None):
    """y = A β(idx) + noise, β one-hot with c_l at idx[b, l] (sparc_ldpc.py:436-446)."""
    x, _ = column_sum(ordering, M, n, Pl, idx)
    return x if noise is None else x + _ld(noise).reshape(x.shape)


def cancel(ordering, M, n, Pl, y, idx, scale=1.0, sections=None):
    """y − scale · A β(idx) over the decided sections (sparc_ldpc.py:508-518;
    amp_exit.py:107-111 with idx −1 = keep).  ``sections``: the section each
    column of idx belongs to (default: all L)."""
    x, _ = column_sum(ordering, M, n, Pl, idx, sections)
    return _ld(y).reshape(x.shape) - LD(scale) * x


def onehot(n, Pl, M, idx, scale=1.0):
    """β₀ (B, L·M): scale · c_l at idx[b, l], 0 elsewhere; idx −1 = an all-zero
    section (sparc_ldpc.py:832-835)."""
    idx = np.asarray(idx, dtype=np.int64)
    B, L = idx.shape
    c = coeffs(n, Pl) * LD(scale)
    out = np.zeros((B, L, M), dtype=LD)
    b, l = np.nonzero(idx >= 0)
    out[b, l, idx[b, l]] = c[l]
    return out.reshape(B, L * M)


def sp2bp(post, L, M):
    """p_t = P(bit t = 1): the entries whose bit t is set, added one by one in
    ascending index order, MSB first per section (the loop of
    sparc_ldpc.py:257-281, ``p[b] = p[b] + bl[j]``).  The accumulator has the
    dtype of ``post``: binary64 input gives the reference's p bit for bit (its
    rounding is part of what the LLR of a p near 1 is), long double input the
    sum to long double accuracy.  post (..., L·M) -> (..., L·log2 M)."""
    lgm = _lgm(M)
    post = np.asarray(post)
    assert post.dtype in (np.float64, LD)
    lead = post.shape[:-1]
    sec = post.reshape(lead + (L, M))
    j = np.arange(M)
    p = np.empty(lead + (L, lgm), dtype=post.dtype)
    for t in range(lgm):
        sel = sec[..., ((j >> (lgm - 1 - t)) & 1) == 1]
        p[..., t] = np.add.accumulate(sel, axis=-1)[..., -1]  # strictly left to right
    return p.reshape(lead + (L * lgm,))


def llr_of_p(p):
    """nan_to_num(log(1 − p) − log p) as binary64 does it (sparc_ldpc.py:478-479):
    ±inf -> ±finfo(float64).max, NaN -> 0."""
    p = _ld(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(LD(1) - p) - np.log(p)
    out = np.where(np.isnan(v), LD(0), v)
    out = np.where(np.isposinf(v), LD(F64_MAX), out)
    out = np.where(np.isneginf(v), -LD(F64_MAX), out)
    return out


def llr(beta, n, Pl, L, M, l0, ns):
    """LLRs of the LDPC bits of sections [l0, l0 + ns) of β (B, L·M)
    (sparc_ldpc.py:470-479): the posterior β / c_l and p in binary64 as the
    reference forms them, the two logarithms in long double.
    -> (llr long double, p binary64), both (B, ns·log2 M)."""
    beta = np.asarray(beta, dtype=np.float64)
    B = beta.shape[0]
    post = beta.reshape(B, L, M) / coeffs(n, Pl).astype(np.float64)[None, :, None]
    p = sp2bp(np.ascontiguousarray(post[:, l0:l0 + ns]).reshape(B, ns * M), ns, M)
    return llr_of_p(p), p


def bp2sp(bp, L, M):
    """Section posteriors from bit marginals bp_t = P(bit t = 1), MSB first:
    sp_m = Π_t (bit_t(m) ? bp_t : 1 − bp_t), normalised per section
    (sparc_ldpc.py:283-314).  bp (..., L·log2 M) -> (..., L·M)."""
    lgm = _lgm(M)
    bp = _ld(bp)
    lead = bp.shape[:-1]
    b = bp.reshape(lead + (L, lgm))
    m = np.arange(M)
    sp = np.ones(lead + (L, M), dtype=LD)
    for t in range(lgm):
        bit = ((m >> (lgm - 1 - t)) & 1) == 1
        sp = sp * np.where(bit, b[..., t:t + 1], LD(1) - b[..., t:t + 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        sp = sp / sp.sum(axis=-1, keepdims=True)
    return sp.reshape(lead + (L * M,))


def bit_marginals(app):
    """bp_t = 1 / (1 + exp(app_t)) (sparc_ldpc.py:683-686, :987-990)."""
    with np.errstate(over="ignore"):
        return LD(1) / (LD(1) + np.exp(_ld(app)))


def soft_sections(app, ns, M):
    """bp2sp of the LDPC a-posteriori LLRs: (B, ns·log2 M) -> (B, ns·M)."""
    return bp2sp(bit_marginals(app), ns, M)


def rescale(beta, n, Pl, L, M):
    """(β / c_l) · c_l, the β₀ of the sections AMP keeps (sparc_ldpc.py:657, :691, :696)."""
    beta = _ld(beta)
    B = beta.shape[0]
    c = coeffs(n, Pl)[None, :, None]
    return ((beta.reshape(B, L, M) / c) * c).reshape(B, L * M)


def soft_beta0(beta, app, n, Pl, L, M, l0, ns):
    """β₀ = β with sections [l0, l0 + ns) replaced by c_l · bp2sp(app)
    (sparc_ldpc.py:683-698); the other sections go through ``rescale``."""
    B = np.asarray(beta).shape[0]
    out = rescale(beta, n, Pl, L, M).reshape(B, L, M)
    sp = soft_sections(app, ns, M).reshape(B, ns, M)
    out[:, l0:l0 + ns] = sp * coeffs(n, Pl)[None, l0:l0 + ns, None]
    return out.reshape(B, L * M)


def hard_indices(app, M):
    """Hard decisions of the LDPC output: bits = app < 0, MSB first
    (sparc_ldpc.py:486-490).  (B, ns·log2 M) -> (B, ns) int64."""
    lgm = _lgm(M)
    app = np.asarray(app, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bits = (app < 0).reshape(app.shape[0], -1, lgm).astype(np.int64)
    return (bits << np.arange(lgm - 1, -1, -1)).sum(axis=-1)


def threshold_indices(app, ns, M, thr):
    """Threshold decisions (amp_exit.py:56-105 on the bp2sp of
    sparc_ldpc.py:987-994): a section is decided, with index m, iff exactly one
    entry of its normalised posterior exceeds ``thr``; else −1.
    -> (idx (B, ns) int64, sp (B, ns, M))."""
    sp = soft_sections(app, ns, M)
    B = sp.shape[0]
    sp = sp.reshape(B, ns, M)
    with np.errstate(invalid="ignore"):
        above = sp > LD(thr)
    idx = np.where(above.sum(axis=-1) == 1, above.argmax(axis=-1), -1).astype(np.int64)
    return idx, sp
