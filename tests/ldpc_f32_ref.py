"""The binary32 layered belief-propagation decoders in NumPy: the parity target
of the HIP kernel k_bpl32 (LB_F32).  Test infrastructure only:
the product never imports this module.

The schedule is tests/ldpc_layered_ref.py's, with every quantity held and
rounded in binary32:

    app = ch32(ch) = float32(clip(ch, -2^100, 2^100));  r = 0        (float32)
    for it in 0 .. max_iter-1:
        if stop(app): return float64(app), it
        for each layer, in order:
            q[e] = app[v] - r[e]
            r[edges of c] = check rule on q[edges of c]
            app[v] = q[e] + r[e]
    return float64(app), max_iter

The clamp keeps NaN and the sign of zero.  It is there for saturated inputs:
the library takes variable degrees up to 255, so |app| <= 256 * 2^100 < 2^128
stays finite and inf - inf never arises from LLRs at +-DBL_MAX or +-inf.

The check rule is Lxfb (the loop structure of oracle.ldpc_oracle.lxfb) over

    Lxor32(a, b) = sign * min(|a|, |b|) + c(|a + b|) - c(|a - b|),
    c(x) = log(1 + exp(-x)),

every operation rounded to binary32 ("sumprod2"), or without the c terms and
the outputs times float32(corr_factor) ("minsum": subtract, add, |.|, min, sign
and one multiply, all exact IEEE operations, so a kernel must give the same
bits).  stop(app) is the binary64 schedule's: every check has an even number
of variables with app < 0 and none with app == 0 or NaN.

c has two evaluations.  c_f32: exp, 1 + . and log each in binary32 with NumPy's
float32 routines (the decoder's statement).  c_rounded: in binary64 and rounded
to binary32 once (correctly rounded).  How far a word's app moves between the
two is the conditioning figure P the GPU tests take their bar from.
"""
import numpy as np

import ldpc_layered_ref as lr
from oracle import ldpc_oracle as lo

ALGOS = lr.ALGOS
F = np.float32
CLAMP = 2.0 ** 100


def ch32(ch):
    """float32(clip(ch, -2^100, 2^100)): NaN stays NaN, the sign of zero is kept."""
    ch = np.asarray(ch, dtype=np.float64)
    with np.errstate(invalid="ignore", under="ignore"):
        return np.clip(ch, -CLAMP, CLAMP).astype(np.float32)


def c_f32(x):
    """log(1 + exp(-x)) with every step in binary32."""
    assert x.dtype == np.float32
    with np.errstate(under="ignore", invalid="ignore"):
        return np.log(F(1) + np.exp(-x))


def c_rounded(x):
    """log(1 + exp(-x)) in binary64, rounded to binary32 once."""
    assert x.dtype == np.float32
    with np.errstate(under="ignore", invalid="ignore"):
        return np.log1p(np.exp(-x.astype(np.float64))).astype(np.float32)


def lxor32(a, b, corr=True, c=c_f32):
    assert a.dtype == np.float32 and b.dtype == np.float32
    s = np.where(np.signbit(a) == np.signbit(b), F(1), F(-1))
    L = s * np.fmin(np.abs(a), np.abs(b))
    if corr:
        with np.errstate(invalid="ignore"):
            L = L + c(np.abs(a + b))
            L = L - c(np.abs(a - b))
    assert L.dtype == np.float32
    return L


def decode(ch, vdeg, cdeg, intrlv, first_check, algo="sumprod2", corr_factor=0.7, max_it=lo.MAX_ITCOUNT,
           trace=False, rounded=False, layers=None):
    """(app float64, it) as ldpc_layered_ref.decode; trace=True adds (apps,
    margins): float64(app) and the smallest non-zero |app| at every stop test
    made, the final app appended when the word ran out.  rounded=True
    evaluates c with c_rounded."""
    if algo not in ALGOS:
        raise NameError("Decoder type unknonwn")
    g = layers or lr.Layers(vdeg, cdeg, intrlv, first_check)
    corr = algo == "sumprod2"
    c = c_rounded if rounded else c_f32
    cf = F(corr_factor)

    def rule(Lm):
        lr._lxfb_with(Lm, corr, lambda a, b, co: lxor32(a, b, co, c))
        return Lm if corr else Lm * cf

    app = ch32(ch)
    r = np.zeros(len(g.var_of), dtype=np.float32)
    apps, margins = [], []

    def out(it):
        a64 = app.astype(np.float64)
        if not trace:
            return a64, it
        if it == max_it:
            apps.append(a64)
        return a64, it, np.array(apps).reshape(len(apps), len(app)), np.array(margins)

    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(max_it):
            if trace:
                apps.append(app.astype(np.float64))
                nz = np.abs(app[(app != 0) & ~np.isnan(app)])
                margins.append(float(nz.min()) if len(nz) else np.inf)
            if g.stop(app):
                return out(it)
            for by_deg in g.groups:
                for E, V in by_deg:
                    q = app[V] - r[E]
                    rn = rule(q.copy())
                    assert q.dtype == np.float32 and rn.dtype == np.float32
                    r[E] = rn
                    app[V] = q + rn
    return out(max_it)


truncated = lr.truncated


def decode_code(c, ch, algo="sumprod2", **kw):
    return decode(ch, c.vdeg, c.cdeg, c.intrlv, lr.code_layers(c), algo, **kw)
