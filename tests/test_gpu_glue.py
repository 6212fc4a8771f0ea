"""The SPARC <-> LDPC glue kernels of sa_glue.hip, each entry point by itself
against oracle/glue_oracle.py (long double, pinned to the reference's fixtures
by tests/test_glue_oracle.py), in both precisions, at the smallest geometries
that reach each path: n not a multiple of the 256-row block, L not a multiple
of the four-section group, section ranges that start and end inside a group,
M = 2 ... 4096, and a power allocation in which every c_l differs
(Pl_l ∝ 2^(-l/L), ΣPl = 2).  No AMP decode runs except in the lanes tests.

Bounds (ε = 2^-52):
  k_colsum outputs   |got - ref| <= 4 L ε (|scale| Σ c_l/√n + |base or noise|), the Σ over the sections
                     summed (L sequential binary64 additions, a multiply, a divide, an add);
                     binary32: + 2^-23 |ref| for the one output rounding.
  one-hot β₀         non-zeros within 2 ulp (working type) of scale √(n Pl_l); zeros exact.
  llr                |got - ref| <= 64 ε (|log p| + |log(1 - p)|) where min(p, 1 - p) >= 1e-6 (asserted on
                     the oracle): p itself is the reference's ordered binary64 sum on both sides, the
                     bound covers the two device logarithms.  Saturated inputs: exact.
  soft β₀            inside the range rtol 1e-10 (binary32: 1 ulp of the rounded oracle); outside it 2 ulp
                     (working type) of the staged value; ±800 inputs: exact.
  indices            exact (hard decisions; threshold decisions where min |sp - thr| >= 1e-6).

Every case records max |got - ref| / bound; with SPARC_GLUE_REPORT=<file> the
largest fraction per entry point and precision is written there as JSON.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

from oracle import amp_oracle as orc
from oracle import glue_oracle as go

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
F64_MAX = np.finfo(np.float64).max
PRECS = ["fp32", "fp64"]

# (L, M, n, B, section ranges (l0, ns))
GEOMS = [
    (10, 16, 300, 3, [(0, 10), (3, 6), (9, 1)]),  # n % 256, L % 4, ranges off the group of 4, sections on both sides
    (12, 2, 20, 2, [(0, 12), (5, 4)]),            # lg M = 1: one lane, one term
    (6, 32, 257, 1, [(2, 4)]),                    # M/2 = 16: one unrolled chunk; one row past a 256-row block
    (5, 128, 70, 2, [(1, 3)]),                    # two 64-lane strides, four chunks
    (3, 4096, 40, 2, [(0, 3), (1, 1)]),           # 32 KB LDS section, 16 strides of 256 in k_threshold, n < M
]
GEOM_IDS = [f"L{g[0]}-M{g[1]}-n{g[2]}" for g in GEOMS]
RANGED = [(g, r) for g in GEOMS for r in g[4]]
RANGED_IDS = [f"L{g[0]}-M{g[1]}-n{g[2]}-l{r[0]}+{r[1]}" for g, r in RANGED]
LLR_SCALE = {2: 2.0, 16: 3.0, 32: 4.0, 128: 4.0, 4096: 8.0}
THR_SCALE = {2: 1.5, 16: 3.0, 32: 3.0, 128: 4.0, 4096: 5.0}
# Seeds of the threshold draws, per (M, l0, ns, thr): searched upwards from 0 until
# the ORACLE's decisions hold a decided and an undecided section and no
# posterior lies within 1e-6 of the threshold (both asserted in the test).
THR_SEEDS = {
    (16, 0, 10, 0.3): 0, (16, 0, 10, 0.7): 0, (16, 3, 6, 0.3): 0, (16, 3, 6, 0.7): 0, (16, 9, 1, 0.3): 0,
    (16, 9, 1, 0.7): 0, (2, 0, 12, 0.3): 0, (2, 0, 12, 0.7): 0, (2, 5, 4, 0.3): 0, (2, 5, 4, 0.7): 0,
    (32, 2, 4, 0.3): 0, (32, 2, 4, 0.7): 0, (128, 1, 3, 0.3): 0, (128, 1, 3, 0.7): 0, (4096, 0, 3, 0.3): 0,
    (4096, 0, 3, 0.7): 3, (4096, 1, 1, 0.3): 1, (4096, 1, 1, 0.7): 22,
}


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


# ---- shared set-up ---------------------------------------------------------------

_ORDER, _OPS, _HEADROOM = {}, {}, {}


def power(L, P=2.0):
    pl = 2.0 ** (-np.arange(L) / L)
    return pl * (P / pl.sum())


def ordering(sp, L, M, n):
    if (L, M, n) not in _ORDER:
        _ORDER[(L, M, n)] = np.array(sp.make_ordering(L, M, n))
    return _ORDER[(L, M, n)]


def operator(sp, L, M, n, prec, tag="a", B=3, staged=True):
    """A cached operator per (shape, precision, tag), B codewords reserved, Pl staged."""
    key = (L, M, n, prec, tag)
    if key not in _OPS:
        op = sp.SparcOperator(L, M, n, ordering(sp, L, M, n), precision=prec)
        op.reserve(max(B, 3), 1)
        if staged:
            op.stage_power(max(B, 3), power(L))
        _OPS[key] = op
    return _OPS[key]


def wt(prec):
    return np.float32 if prec == "fp32" else np.float64


def ulp(x, prec):
    """Spacing of the working type at x (x already a value of that type, or rounded to it)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(wt(prec))).astype(np.float64)


def record(entry, prec, err, bound):
    """Keep the largest err / bound of an entry point and precision; returns the fractions."""
    err = np.asarray(err, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = float(frac.max()) if frac.size else 0.0
    _HEADROOM[(entry, prec)] = max(_HEADROOM.get((entry, prec), 0.0), worst)
    print(f"{entry} [{prec}]: max err {float(err.max()) if err.size else 0.0:.3e}, worst err/bound {worst:.3e}")
    return frac


@pytest.fixture(scope="module", autouse=True)
def headroom_report():
    yield
    path = os.environ.get("SPARC_GLUE_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{k[0]}|{k[1]}": v for k, v in sorted(_HEADROOM.items())}, fh, indent=1)
    _OPS.clear()


def colsum_check(entry, prec, L, got, ref, mag, other, scale=1.0):
    """The k_colsum bound of the module docstring; mag (B,), other (B, n) = |base| or |noise|."""
    ref64 = np.asarray(ref, dtype=np.float64)
    bound = 4 * L * EPS * (abs(scale) * np.asarray(mag, dtype=np.float64)[:, None] + np.abs(other))
    if prec == "fp32":
        bound = bound + 2.0 ** -23 * np.abs(ref64)
    err = np.abs(np.asarray(go.LD(1) * got - ref, dtype=np.float64))
    frac = record(entry, prec, err, bound)
    assert np.all(frac <= 1.0), (entry, prec, float(frac.max()))


def draw_idx(rs, B, L, M):
    idx = rs.randint(0, M, (B, L)).astype(np.int32)
    idx[0, 0], idx[0, 1] = 0, M - 1
    idx[B - 1, L - 1] = M - 1
    return idx


# ---- 0. fetch_y ------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_fetch_y_returns_the_staged_y(sp, prec):
    L, M, n, B, _ = GEOMS[0]
    op = operator(sp, L, M, n, prec)
    y = np.random.RandomState(1).randn(B, n)
    op.stage(y)
    assert np.array_equal(op.fetch_y(B), y.astype(wt(prec)).astype(np.float64))
    assert np.array_equal(op.fetch_y(1), y[:1].astype(wt(prec)).astype(np.float64))
    y2 = np.random.RandomState(2).randn(1, n)
    op.stage(y2)  # one codeword: the others keep theirs
    want = np.concatenate([y2, y[1:]]).astype(wt(prec)).astype(np.float64)
    assert np.array_equal(op.fetch_y(B), want)


# ---- 1. encode -------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_encode(sp, geom, prec):
    L, M, n, B, _ = geom
    op, Pl, o = operator(sp, L, M, n, prec), power(L), ordering(sp, L, M, n)
    rs = np.random.RandomState(10 + M)
    idx = draw_idx(rs, B, L, M)
    noise = rs.randn(B, n) * 0.7
    x, mag = go.column_sum(o, M, n, Pl, idx)
    op.encode(idx, noise)
    colsum_check("encode(idx, noise)", prec, L, op.fetch_y(B), x + noise.astype(go.LD), mag, np.abs(noise))
    op.encode(idx)
    got = op.fetch_y(B)
    colsum_check("encode(idx)", prec, L, got, x, mag, np.zeros((B, n)))
    # different codewords, and every row written: y is ± sums of L non-zero terms
    assert B == 1 or not np.array_equal(got[0], got[1])


# ---- 2. cancel -------------------------------------------------------------------

@pytest.mark.parametrize("scale", [None, 0.37])
@pytest.mark.parametrize("inplace", [False, True], ids=["dst", "inplace"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_cancel(sp, geom, prec, inplace, scale):
    """Three codewords whatever the geometry's B: about a third of the entries
    -1, codeword 1 all -1 (y unchanged, exactly), codeword 2 with no -1."""
    L, M, n, _, _ = geom
    B = 3
    src, Pl, o = operator(sp, L, M, n, prec), power(L), ordering(sp, L, M, n)
    dst = src if inplace else operator(sp, L, M, n, prec, tag="b")
    rs = np.random.RandomState(20 + M)
    idx = draw_idx(rs, B, L, M)
    idx[0, rs.rand(L) < 0.5] = -1
    idx[0, 0], idx[0, 1] = 0, -1  # both kinds whatever the draw
    idx[1, :] = -1
    y = rs.randn(B, n)
    src.stage(y)
    base = src.fetch_y(B)  # the values the device holds (binary32: y rounded)
    if not inplace:
        dst.stage(np.full((B, n), 7.0))
    s = 1.0 if scale is None else scale
    x, mag = go.column_sum(o, M, n, Pl, idx)
    ref = base.astype(go.LD) - go.LD(s) * x
    src.cancel(idx, dst, scale)
    got = dst.fetch_y(B)
    colsum_check("cancel(scale)" if scale else "cancel", prec, L, got, ref, mag, np.abs(base), s)
    assert np.array_equal(got[1], base[1])
    assert not np.array_equal(got[2], base[2])
    if not inplace:
        assert np.array_equal(src.fetch_y(B), base)


# ---- 3. hard decisions and hard cancellation ---------------------------------------

def special_app(rs, B, ns, lgm):
    app = rs.randn(B, ns * lgm) * 3
    spec = [0.0, -0.0, np.nan, np.inf, -np.inf, F64_MAX, -F64_MAX]
    pos = rs.permutation(app.size)[:len(spec)] if app.size >= 2 * len(spec) else np.arange(min(app.size, len(spec)))
    app.reshape(-1)[pos] = spec[:len(pos)]
    return app


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom,rng", RANGED, ids=RANGED_IDS)
def test_hard_cancel(sp, geom, rng, prec):
    L, M, n, B, _ = geom
    l0, ns = rng
    lgm = int(np.log2(M))
    src, Pl, o = operator(sp, L, M, n, prec), power(L), ordering(sp, L, M, n)
    rs = np.random.RandomState(30 + M + l0)
    app = special_app(rs, B, ns, lgm)
    want = go.hard_indices(app, M)
    y = rs.randn(B, n)
    src.stage(y)
    base = src.fetch_y(B)
    idx = src.hard_cancel(B, l0, ns, app)
    assert idx.dtype == np.int32 and np.array_equal(idx, want)
    assert np.array_equal(src.fetch_y(B), base)  # no dst: y untouched
    # with dst: the shortened operator over the sections before the LDPC ones, as the joint decoder; else a second full one
    key = (L, M, n, prec, "sub", l0)
    if l0 > 0:
        if key not in _OPS:
            _OPS[key] = src.subset(range(l0))
        dst = _OPS[key]
    else:
        dst = operator(sp, L, M, n, prec, tag="b")
    idx2 = src.hard_cancel(B, l0, ns, app, dst=dst)
    assert np.array_equal(idx2, want)
    x, mag = go.column_sum(o, M, n, Pl, want, sections=np.arange(l0, l0 + ns))
    colsum_check("hard_cancel(dst)", prec, L, dst.fetch_y(B), base.astype(go.LD) - x, mag, np.abs(base))
    assert np.array_equal(src.fetch_y(B), base)


# ---- 4. one-hot β₀ -------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_stage_onehot(sp, geom, prec):
    L, M, n, B, _ = geom
    op, Pl = operator(sp, L, M, n, prec), power(L)
    rs = np.random.RandomState(40 + M)
    idx = draw_idx(rs, B, L, M)
    part = idx.copy()
    part[0, 2] = -1
    part[B - 1, rs.rand(L) < 0.4] = -1
    for name, ix, scale in (("stage_onehot", idx, None), ("stage_onehot(scale)", part, 0.37),
                            ("stage_onehot(scale)", part, -1.5)):
        op.stage(np.zeros((B, n)), None, np.full((B, L * M), 3.0))  # stale β everywhere
        op.stage_onehot(ix, scale)
        got = op.fetch(B)[0]
        ref = go.onehot(n, Pl, M, ix, 1.0 if scale is None else scale)
        nz = np.asarray(ref != 0)
        assert nz.sum() == (ix >= 0).sum()
        assert np.all(got[~nz] == 0.0)
        ref64 = np.asarray(ref, dtype=np.float64)
        err = np.abs(np.asarray(go.LD(1) * got - ref, dtype=np.float64))[nz]
        frac = record(name, prec, err, 2 * ulp(ref64[nz], prec))
        assert np.all(frac <= 1.0), (name, prec, float(frac.max()))


# ---- 5. sp2bp + LLR --------------------------------------------------------------------

def soft_beta(rs, B, L, M, n, Pl, s):
    g = rs.randn(B, L, M) * s
    e = np.exp(g - g.max(axis=2, keepdims=True))
    return (np.sqrt(n * Pl)[None, :, None] * e / e.sum(axis=2, keepdims=True)).reshape(B, L * M)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom,rng", RANGED, ids=RANGED_IDS)
def test_llr_regular(sp, geom, rng, prec):
    L, M, n, B, _ = geom
    l0, ns = rng
    op, Pl = operator(sp, L, M, n, prec), power(L)
    beta = soft_beta(np.random.RandomState(50 + M), B, L, M, n, Pl, LLR_SCALE[M])
    op.stage(np.zeros((B, n)), Pl, beta)
    held = beta.astype(wt(prec)).astype(np.float64)
    assert np.array_equal(op.fetch(B)[0], held)
    ref, p = go.llr(held, n, Pl, L, M, l0, ns)
    assert np.minimum(p, 1 - p).min() >= 1e-6, "precondition: no LLR near saturation"
    got = op.llr(B, l0, ns)
    assert got.shape == ref.shape
    bound = 64 * EPS * (np.abs(np.log(p)) + np.abs(np.log1p(-p)))
    frac = record("llr", prec, np.abs(np.asarray(go.LD(1) * got - ref, dtype=np.float64)), bound)
    assert np.all(frac <= 1.0), float(frac.max())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom,rng", RANGED, ids=RANGED_IDS)
def test_llr_saturated(sp, geom, rng, prec):
    """Decided, empty and overfull sections: exact LLRs.  A one-hot section at c_l
    (in binary32: c_l rounded, what AMP leaves in a decided section) has p in
    {0, 1}: -max on the index's set bits, +max on the others; an all-zero section
    +max everywhere; 1.001 c_l at one entry has p > 1 there: log(1 - p) is NaN,
    which nan_to_num turns into 0 (the reference's behaviour), +max on the others."""
    L, M, n, B, _ = geom
    l0, ns = rng
    lgm = int(np.log2(M))
    op, Pl = operator(sp, L, M, n, prec), power(L)
    c = np.sqrt(n * Pl)
    rs = np.random.RandomState(60 + M)
    at = draw_idx(rs, B, L, M)
    kind = (np.arange(B)[:, None] + np.arange(L)[None, :]) % 3  # 0 one-hot, 1 empty, 2 overfull
    beta = np.zeros((B, L, M))
    want = np.empty((B, L, lgm))
    for b in range(B):
        for l in range(L):
            bits = (at[b, l] >> np.arange(lgm - 1, -1, -1)) & 1
            if kind[b, l] == 0:
                beta[b, l, at[b, l]] = c[l]
                want[b, l] = np.where(bits == 1, -F64_MAX, F64_MAX)
            elif kind[b, l] == 1:
                want[b, l] = F64_MAX
            else:
                beta[b, l, at[b, l]] = 1.001 * c[l]
                want[b, l] = np.where(bits == 1, 0.0, F64_MAX)
    op.stage(np.zeros((B, n)), Pl, beta.reshape(B, L * M))
    got = op.llr(B, l0, ns)
    assert np.array_equal(got, want[:, l0:l0 + ns].reshape(B, ns * lgm))
    assert not np.signbit(got[got == 0.0]).any()


# ---- 6. bp2sp into β₀ -------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom,rng", RANGED, ids=RANGED_IDS)
def test_soft_beta0(sp, geom, rng, prec):
    L, M, n, B, _ = geom
    l0, ns = rng
    lgm = int(np.log2(M))
    op, Pl = operator(sp, L, M, n, prec), power(L)
    rs = np.random.RandomState(70 + M + l0)
    app = np.clip(rs.randn(B, ns * lgm) * 3, -6, 6)
    op.stage(np.zeros((B, n)), Pl, rs.rand(B, L * M) + 0.05)
    staged = op.fetch(B)[0]
    assert staged.min() > 0
    op.soft_beta0(B, l0, ns, app)
    got = op.fetch(B)[0].reshape(B, L, M)
    ref = go.soft_beta0(staged, app, n, Pl, L, M, l0, ns).reshape(B, L, M)
    ref64 = np.asarray(ref, dtype=np.float64)
    inside = np.zeros(L, dtype=bool)
    inside[l0:l0 + ns] = True
    err = np.abs(np.asarray(go.LD(1) * got - ref, dtype=np.float64))
    if prec == "fp64":
        frac = record("soft_beta0 (range)", prec, err[:, inside], 1e-10 * np.abs(ref64[:, inside]))
    else:
        r32 = ref64.astype(np.float32).astype(np.float64)
        frac = record("soft_beta0 (range)", prec, np.abs(got - r32)[:, inside], ulp(r32[:, inside], prec))
    assert np.all(frac <= 1.0), float(frac.max())
    # per section the posteriors sum to c_l
    tol = 1e-12 if prec == "fp64" else 1e-6
    np.testing.assert_allclose(got[:, inside].sum(axis=2), np.tile(np.sqrt(n * Pl)[inside], (B, 1)), rtol=tol)
    if (~inside).any():
        st = staged.reshape(B, L, M)[:, ~inside]
        frac = record("soft_beta0 (kept sections)", prec, np.abs(got[:, ~inside] - st), 2 * ulp(st, prec))
        assert np.all(frac <= 1.0), float(frac.max())
    else:
        assert (l0, ns) == (0, L)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom,rng", RANGED, ids=RANGED_IDS)
def test_soft_beta0_saturated(sp, geom, rng, prec):
    """Every bit at ±800: exactly c_l (as the working type) at the section's index, exactly 0 elsewhere."""
    L, M, n, B, _ = geom
    l0, ns = rng
    lgm = int(np.log2(M))
    op, Pl = operator(sp, L, M, n, prec), power(L)
    rs = np.random.RandomState(80 + M)
    at = draw_idx(rs, B, L, M)[:, l0:l0 + ns]
    bits = (at[:, :, None] >> np.arange(lgm - 1, -1, -1)) & 1
    app = np.where(bits == 1, -800.0, 800.0).reshape(B, ns * lgm)
    op.stage(np.zeros((B, n)), Pl, np.full((B, L * M), 0.5))
    op.soft_beta0(B, l0, ns, app)
    got = op.fetch(B)[0].reshape(B, L, M)[:, l0:l0 + ns]
    want = np.zeros((B, ns, M))
    cw = np.sqrt(n * Pl).astype(wt(prec)).astype(np.float64)
    for b in range(B):
        want[b, np.arange(ns), at[b]] = cw[l0:l0 + ns]
    assert np.array_equal(got, want)


# ---- 7. threshold decisions -----------------------------------------------------------------

def threshold_case(M, B, l0, ns, thr):
    lgm = int(np.log2(M))
    rs = np.random.RandomState(THR_SEEDS[(M, l0, ns, thr)])
    app = rs.randn(B, ns * lgm) * THR_SCALE[M]
    idx, spv = go.threshold_indices(app, ns, M, thr)
    return app, idx, spv


@pytest.mark.parametrize("thr", [0.3, 0.7])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom,rng", RANGED, ids=RANGED_IDS)
def test_threshold(sp, geom, rng, prec, thr):
    L, M, n, B, _ = geom
    l0, ns = rng
    op = operator(sp, L, M, n, prec)
    app, want, spv = threshold_case(M, B, l0, ns, thr)
    margin = float(np.abs(np.asarray(spv, dtype=np.float64) - thr).min())
    print(f"threshold M={M} thr={thr}: decided {int((want >= 0).sum())} of {want.size}, min |sp - thr| {margin:.2e}")
    assert margin >= 1e-6, "precondition: no posterior an ulp of exp away from the threshold"
    assert (want >= 0).any() and (want < 0).any(), "precondition: a decided and an undecided section"
    got = op.threshold(B, l0, ns, app, thr)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # a NaN app: that section is undecided, the others as before
    b, j = np.argwhere(want >= 0)[0]
    bad = app.copy()
    bad[b, j * int(np.log2(M))] = np.nan
    want2 = want.copy()
    want2[b, j] = -1
    assert np.array_equal(op.threshold(B, l0, ns, bad, thr), want2)


def test_threshold_cases_reach_every_branch():
    """Across the cases above the oracle sees sections with 0, 1 and >= 2 entries above the threshold."""
    seen = set()
    for (L, M, n, B, _), (l0, ns) in RANGED:
        for thr in (0.3, 0.7):
            _, _, spv = threshold_case(M, B, l0, ns, thr)
            seen |= set(np.minimum((spv > thr).sum(axis=-1), 2).reshape(-1).tolist())
    assert seen == {0, 1, 2}


# ---- 8. device-pointer arguments ---------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_device_pointer_arguments(sp, prec):
    """llr(out=ptr), soft_beta0(app=ptr) and hard_cancel(app=ptr) on the LDPC
    context's buffers (L = 64, M = 16, l0 = 16: the 192 bits of 802.16 5/6
    z = 8): bit-identical to the host-pointer forms."""
    L, M, n, l0, ns, B = 64, 16, 256, 16, 48, 2
    code = sp.code("802.16", "5/6", 8)
    d_ch, d_app, _ = code.device_buffers(B)
    assert code.N == ns * 4
    op, Pl = operator(sp, L, M, n, prec), power(L)
    sub = op.subset(range(l0))
    rs = np.random.RandomState(7)
    beta = soft_beta(rs, B, L, M, n, Pl, 3.0)
    y = rs.randn(B, n)
    op.stage(y, Pl, beta)
    host = op.llr(B, l0, ns)
    assert np.isfinite(host).all() and np.abs(host).max() < 1e300
    op.llr(B, l0, ns, out=d_app)  # lands where fetch_buffers reads
    dev, _ = code.fetch_buffers(B)
    assert np.array_equal(dev, host)
    # app = those LLRs, from the host and from the device buffer
    idx_h = op.hard_cancel(B, l0, ns, host, dst=sub)
    y_h = sub.fetch_y(B)
    sub.stage(np.zeros((B, n)))
    idx_d = op.hard_cancel(B, l0, ns, d_app, dst=sub)
    assert np.array_equal(idx_d, idx_h) and np.array_equal(idx_h, go.hard_indices(host, M))
    assert np.array_equal(sub.fetch_y(B), y_h) and not np.array_equal(y_h, np.zeros((B, n)))
    op.soft_beta0(B, l0, ns, host)
    b_h = op.fetch(B)[0]
    op.stage(y, Pl, beta)
    op.soft_beta0(B, l0, ns, d_app)
    assert np.array_equal(op.fetch(B)[0], b_h)
    assert not np.array_equal(b_h, beta.astype(wt(prec)).astype(np.float64))


# ---- 9. glue on a context whose lanes are live ---------------------------------------------------

LANE_SHAPE, LANE_T = (16, 16, 96), 4
_LANE_IN = {}


def lane_inputs():
    if not _LANE_IN:
        L, M, n = LANE_SHAPE
        Pl = power(L)
        Ab = orc.sparc_transforms(L, M, n)[0]
        rs = np.random.RandomState(77)
        _LANE_IN.update(
            Pl=Pl, ys=[orc.rep_inputs(L, M, n, Pl, 0.6, Ab, 900 + i)[1].reshape(1, -1) for i in range(2)],
            app=np.clip(rs.randn(1, 12 * 4) * 3, -6, 6), idx=rs.randint(0, M, (1, L)).astype(np.int32),
            noise=rs.randn(1, n) * 0.6, part=np.where(rs.rand(1, L) < 0.4, -1, rs.randint(0, M, (1, L))).astype(np.int32))
    return _LANE_IN


def bring_up(op):
    """test_gpu_decode_lanes.pipelined, two staged steps: the second is issued
    while the first's decide_async is uncollected (it takes the other lane
    where lanes are allowed)."""
    d = lane_inputs()
    op.reserve(1, LANE_T)
    got = []
    for k, y in enumerate(d["ys"]):
        op.stage(y, d["Pl"])
        op.run(1, LANE_T, early_stop=False)
        op.decide_async(1, k % 2)
        if k > 0:
            got.append(op.decide_collect(1, (k - 1) % 2))
    got.append(op.decide_collect(1, (len(d["ys"]) - 1) % 2))
    return got


def glue_sequence(op, cancel_dst=None):
    """The calls of the joint decoder around a decode, each output kept."""
    d = lane_inputs()
    L, M, n = LANE_SHAPE
    out = dict(decisions=bring_up(op))
    out["llr"] = op.llr(1, 4, 12)                                  # 1. describes the latest decode
    sub = op.subset(range(4))
    out["hard_idx"] = op.hard_cancel(1, 4, 12, d["app"], dst=sub)  # 2.
    out["hard_y"] = sub.fetch_y(1)
    op.soft_beta0(1, 4, 12, d["app"])                              # 3.
    out["soft"] = op.fetch(1)[0]
    op.run(1, LANE_T, early_stop=False, beta0=True)                # 4.
    out["run_b0"] = op.fetch(1)
    op.encode(d["idx"], d["noise"])                                # 5.
    out["enc_y"] = op.fetch_y(1)
    op.decide_async(1, 0)                                          # 6. a step outstanding, no re-stage: this run
    op.run(1, LANE_T, early_stop=False)                            #    takes the other lane and must find the encoded y
    out["run_enc"] = op.fetch(1)
    out["dec_b0"] = op.decide_collect(1, 0)
    out["y_after_run"] = op.fetch_y(1)
    dst = op if cancel_dst is None else cancel_dst
    op.cancel(d["part"], dst)                                      # 7.
    out["cancel_y"] = dst.fetch_y(1)
    if cancel_dst is not None:  # the destination decodes what it was handed
        dst.run(1, LANE_T, early_stop=False)
        out["dst_run"] = dst.fetch(1)
    out["bytes"] = op.info()["device_bytes"]
    return out


def flat(v):
    return v if isinstance(v, (tuple, list)) else (v,)


@pytest.mark.parametrize("dst_lanes", [False, True], ids=["inplace", "dst-with-lanes"])
@pytest.mark.parametrize("prec", PRECS)
def test_glue_with_live_lanes(sp, prec, dst_lanes):
    L, M, n = LANE_SHAPE
    o = ordering(sp, L, M, n)

    def make(plan):
        return sp.SparcOperator(L, M, n, o, precision=prec, plan=plan)

    runs = {}
    for name, plan in (("lanes", None), ("one", ("NO_LANES",))):
        op, dst = make(plan), None
        if dst_lanes:
            dst = make(plan)
            dst.stage_power(1, lane_inputs()["Pl"])
            bring_up(dst)
        runs[name] = glue_sequence(op, dst)
        if dst is not None:
            runs[name]["dst_bytes"] = dst.info()["device_bytes"]
    a, b = runs["lanes"], runs["one"]
    for key in b:
        if key.endswith("bytes"):
            continue
        for u, v in zip(flat(a[key]), flat(b[key])):
            assert np.array_equal(np.asarray(u), np.asarray(v)), key
    # the lanes were on: a second set of state buffers, two estimates at the least (test_lanes_stay_off's reading)
    lane = 2 * L * M * (4 if prec == "fp32" else 8)
    assert a["bytes"] - b["bytes"] >= lane, (a["bytes"], b["bytes"])
    if dst_lanes:
        assert a["dst_bytes"] - b["dst_bytes"] >= lane
    # and the sequence is not vacuous: each step changed what the next one read
    d = lane_inputs()
    assert not np.array_equal(b["enc_y"], d["ys"][1].astype(wt(prec)).astype(np.float64))
    assert np.array_equal(b["y_after_run"], b["enc_y"]) and not np.array_equal(b["cancel_y"], b["enc_y"])
    assert not np.array_equal(b["run_enc"][0], b["run_b0"][0])
    # against the oracle too: the LLRs are those of the second decode, the cancelled y that of the encoded one
    Pl = d["Pl"]
    x, mag = go.column_sum(o, M, n, Pl, d["part"])
    colsum_check("cancel (lanes)", prec, L, a["cancel_y"], a["enc_y"].astype(go.LD) - x, mag, np.abs(a["enc_y"]))


# ---- 10. refusals ----------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_refusals_leave_the_staged_inputs_alone(sp, prec):
    L, M, n, B = 10, 16, 300, 2
    lgm = 4
    o = ordering(sp, L, M, n)
    Pl = power(L)
    rs = np.random.RandomState(3)
    y, beta = rs.randn(B, n), rs.rand(B, L * M)
    idx = draw_idx(rs, B, L, M)
    idx3 = draw_idx(rs, 3, L, M)
    op = sp.SparcOperator(L, M, n, o, precision=prec)
    op.reserve(B, 1)
    op.stage(y, Pl, beta)
    other_n = sp.SparcOperator(L, M, n + 1, sp.make_ordering(L, M, n + 1), precision=prec)
    other_p = sp.SparcOperator(L, M, n, o, precision="fp64" if prec == "fp32" else "fp32")
    y0, b0 = op.fetch_y(B), op.fetch(B)[0]

    def refused(call, who=op, yb=(y0, b0)):
        with pytest.raises(sp.SparcAmpError):
            call()
        assert np.array_equal(who.fetch_y(B), yb[0]) and np.array_equal(who.fetch(B)[0], yb[1])

    app = lambda b, ns: rs.randn(b, ns * lgm)  # noqa: E731
    bad_idx, big_idx = idx.copy(), idx.copy()
    bad_idx[1, 3], big_idx[0, 5] = -1, M
    for l0, ns in ((8, 3), (0, L + 1), (L, 1), (2, 0)):  # l0 + ns > L; ns = 0
        refused(lambda: op.llr(B, l0, ns))
        refused(lambda: op.soft_beta0(B, l0, ns, app(B, max(ns, 1))))
        refused(lambda: op.hard_cancel(B, l0, ns, app(B, max(ns, 1))))
        refused(lambda: op.hard_cancel(B, l0, ns, app(B, max(ns, 1)), dst=other_p))
        refused(lambda: op.threshold(B, l0, ns, app(B, max(ns, 1)), 0.5))
    # B above the reserved batch
    refused(lambda: op.llr(3, 2, 4))
    refused(lambda: op.soft_beta0(3, 2, 4, app(3, 4)))
    refused(lambda: op.hard_cancel(3, 2, 4, app(3, 4)))
    refused(lambda: op.threshold(3, 2, 4, app(3, 4), 0.5))
    refused(lambda: op.cancel(idx3, op))
    refused(lambda: op.stage_onehot(idx3))
    refused(lambda: op.stage_onehot(idx3, 0.5))
    refused(lambda: op.fetch_y(3))
    # indices and scales
    refused(lambda: op.stage_onehot(bad_idx))
    refused(lambda: op.stage_onehot(big_idx))
    refused(lambda: op.stage_onehot(big_idx, 0.5))
    refused(lambda: op.stage_onehot(idx, np.inf))
    refused(lambda: op.cancel(idx, op, scale=np.inf))
    refused(lambda: op.cancel(idx, op, scale=np.nan))
    refused(lambda: op.cancel(big_idx, op))
    refused(lambda: op.encode(bad_idx))
    refused(lambda: op.encode(big_idx))
    # destinations of another n / precision
    for other in (other_n, other_p):
        refused(lambda: op.hard_cancel(B, 2, 4, app(B, 4), dst=other))
        refused(lambda: op.cancel(idx, other))
    # glue before stage_power
    raw = sp.SparcOperator(L, M, n, o, precision=prec)
    raw.reserve(B, 1)
    raw.stage(y, None, beta)
    yb = (raw.fetch_y(B), raw.fetch(B)[0])
    assert np.array_equal(yb[0], y0) and np.array_equal(yb[1], b0)
    for call in (lambda: raw.llr(B, 2, 4), lambda: raw.encode(idx), lambda: raw.stage_onehot(idx),
                 lambda: raw.stage_onehot(idx, 0.5), lambda: raw.soft_beta0(B, 2, 4, app(B, 4)),
                 lambda: raw.hard_cancel(B, 2, 4, app(B, 4)), lambda: raw.threshold(B, 2, 4, app(B, 4), 0.5),
                 lambda: raw.cancel(idx, raw)):
        refused(call, raw, yb)
    # M not a power of two
    Lq, Mq, nq = 4, 100, 64
    odd = sp.SparcOperator(Lq, Mq, nq, sp.make_ordering(Lq, Mq, nq), precision=prec)
    odd.reserve(B, 1)
    odd.stage(rs.randn(B, nq), power(Lq), rs.rand(B, Lq * Mq))
    yq = (odd.fetch_y(B), odd.fetch(B)[0])
    iq = rs.randint(0, Mq, (B, Lq)).astype(np.int32)
    for call in (lambda: odd.llr(B, 0, Lq), lambda: odd.encode(iq), lambda: odd.stage_onehot(iq)):
        refused(call, odd, yq)
