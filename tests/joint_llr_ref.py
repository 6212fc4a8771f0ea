"""The two-sided section->bit LLR of the joint decoder (sa_llr_ex,
SA_LLR_TWO_SIDED) stated in NumPy — TEST INFRASTRUCTURE ONLY — and the cases
its CPU and GPU tests share.

Statement, per section l of a β held in the working type ``real``:

  post_j = 1 if β_j == (real) c_l else (double) β_j / c_l      (binary64; c_l = sqrt(n Pl_l))
  p1_t   = Σ post_j over the entries j whose bit (log2 M − 1 − t) is set,
           added one by one in ascending j in binary64 (the reference's p)
  p0_t   = the same over the entries whose bit is clear
  llr_t  = log p0_t − log p1_t (long double), NaN → 0, then
           clip None / 0 / inf: ±inf → ±finfo(float64).max
           clip c > 0:          min(max(llr, −c), c), ±inf → ±c

The geometries, the draws and their scales are those of the LLR tests of
tests/test_gpu_glue.py (copied: test modules do not import each other).
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
F64_MAX = np.finfo(np.float64).max

# (L, M, n, B, section ranges (l0, ns))
GEOMS = [
    (10, 16, 300, 3, [(0, 10), (3, 6), (9, 1)]),
    (12, 2, 20, 2, [(0, 12), (5, 4)]),
    (6, 32, 257, 1, [(2, 4)]),
    (5, 128, 70, 2, [(1, 3)]),
    (3, 4096, 40, 2, [(0, 3), (1, 1)]),
]
GEOM_IDS = [f"L{g[0]}-M{g[1]}-n{g[2]}" for g in GEOMS]
RANGED = [(g, r) for g in GEOMS for r in g[4]]
RANGED_IDS = [f"L{g[0]}-M{g[1]}-n{g[2]}-l{r[0]}+{r[1]}" for g, r in RANGED]
LLR_SCALE = {2: 2.0, 16: 3.0, 32: 4.0, 128: 4.0, 4096: 8.0}
WIDE_SCALE = 30.0  # |LLR| up to about 70: past 16, where a binary32 1 − p is noise
PRECS = ["fp32", "fp64"]


def wt(prec):
    return np.float32 if prec == "fp32" else np.float64


def held(beta, prec):
    """β as the device holds it in the working type, widened again."""
    return np.asarray(beta, dtype=np.float64).astype(wt(prec)).astype(np.float64)


def power(L, P=2.0):
    pl = 2.0 ** (-np.arange(L) / L)
    return pl * (P / pl.sum())


def soft_beta(rs, B, L, M, n, Pl, s):
    g = rs.randn(B, L, M) * s
    e = np.exp(g - g.max(axis=2, keepdims=True))
    return (np.sqrt(n * Pl)[None, :, None] * e / e.sum(axis=2, keepdims=True)).reshape(B, L * M)


def draw(M, B, L, n, scale):
    """The LLR tests' draw of a geometry: RandomState(50 + M), as test_llr_regular."""
    return soft_beta(np.random.RandomState(50 + M), B, L, M, n, power(L), scale)


def finish(v, clip=None):
    """NaN → 0 and the clip (module docstring) of long double LLRs."""
    v = np.asarray(v, dtype=LD)
    out = np.where(np.isnan(v), LD(0), v)
    lim = F64_MAX if clip is None or clip == 0 or np.isinf(clip) else clip
    return np.minimum(np.maximum(out, -LD(lim)), LD(lim))


def two_sided_llr(beta, n, Pl, L, M, l0, ns, prec="fp64", clip=None):
    """β (B, L·M), binary64 values already held in ``prec``'s type
    -> (llr long double, p0 binary64, p1 binary64), each (B, ns·log2 M)."""
    lgm = int(M).bit_length() - 1
    assert M >= 2 and 1 << lgm == M
    beta = np.asarray(beta, dtype=np.float64)
    B = beta.shape[0]
    c = np.sqrt(n * np.asarray(Pl, dtype=np.float64).reshape(-1))
    cr = c.astype(wt(prec)).astype(np.float64)
    sec = beta.reshape(B, L, M)[:, l0:l0 + ns]
    with np.errstate(divide="ignore", invalid="ignore"):
        post = np.where(sec == cr[None, l0:l0 + ns, None], 1.0, sec / c[None, l0:l0 + ns, None])
    j = np.arange(M)
    p0 = np.empty((B, ns, lgm))
    p1 = np.empty((B, ns, lgm))
    for t in range(lgm):
        one = ((j >> (lgm - 1 - t)) & 1) == 1
        p1[..., t] = np.add.accumulate(post[..., one], axis=-1)[..., -1]  # strictly left to right
        p0[..., t] = np.add.accumulate(post[..., ~one], axis=-1)[..., -1]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(p0.astype(LD)) - np.log(p1.astype(LD))
    shape = (B, ns * lgm)
    return finish(v, clip).reshape(shape), p0.reshape(shape), p1.reshape(shape)


def log_bound(p0, p1):
    """64 ε (|log p0| + |log p1|): two binary64 logarithms of the same sums."""
    with np.errstate(divide="ignore"):
        return 64 * EPS * (np.abs(np.log(p0)) + np.abs(np.log(p1)))


def hand_vectors(B, L, M, n, Pl):
    """Decided, empty and overfull sections, kind (b + l) % 3: a one-hot section
    at c_l, an all-zero one, 1.001 c_l at one entry.  -> (β (B, L·M), sign
    (B, L·log2 M)): the two-sided LLR is sign · max (sign · clip): −1 on the set
    bits of a one-hot or overfull section's entry, +1 on its clear bits, 0
    throughout an empty section (0/0; the reference form gives +max there, and
    0 on the set bits of an overfull one)."""
    lgm = int(np.log2(M))
    c = np.sqrt(n * np.asarray(Pl, dtype=np.float64))
    rs = np.random.RandomState(60 + M)
    at = rs.randint(0, M, (B, L))
    at[0, 0], at[0, 1], at[B - 1, L - 1] = 0, M - 1, M - 1
    beta = np.zeros((B, L, M))
    sign = np.zeros((B, L, lgm))
    for b in range(B):
        for l in range(L):
            kind = (b + l) % 3
            if kind == 1:
                continue
            beta[b, l, at[b, l]] = c[l] if kind == 0 else 1.001 * c[l]
            bits = (at[b, l] >> np.arange(lgm - 1, -1, -1)) & 1
            sign[b, l] = np.where(bits == 1, -1.0, 1.0)
    return beta.reshape(B, L * M), sign.reshape(B, L * lgm)
