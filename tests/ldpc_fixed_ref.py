"""Fixed-point layered normalised min-sum in NumPy: the statement the HIP kernel
k_bplq (LB_FIXED) is held to, bit for bit.  Test infrastructure
only: the product never imports this module.

    rmax = 2^(MB-1) - 1;  amax = 2^(AB-1) - 1;  alpha = rint(16 corr_factor) in 1..16
    app[v] = clip(rint(ch[v] 2^F), -rmax, +rmax)      half to even; NaN -> 0; +-inf saturate; -0.0 -> 0
    r[e]   = 0
    for it in 0 .. max_iter-1:
        if stop(app): return app 2^-F, it
        for each layer, in order; for each check c of the layer, edges e on variables v:
            q[e]  = clip(app[v] - r[e], -amax, +amax)
            mag_e = min over the check's other edges e' of |q[e']|      (no other edge: amax)
            neg_e = xor over the check's other edges e' of (q[e'] < 0)
            m     = min((alpha mag_e + 8) >> 4, rmax)
            r[e]  = -m if neg_e else m
            app[v] = clip(q[e] + r[e], -amax, +amax)
    return app 2^-F, max_iter

All of it on integers (int64 here; nothing leaves 17 bits).  stop(app) is the
layered decoders' (ldpc_layered_ref.Layers.stop): every check even in app < 0
and no app == 0.  max_iter = 0 gives (ch, 0), ch untouched.  The checks of a
layer are independent, so the two orders offered (one check at a time, one layer
at a time over its checks of equal degree) must agree bit for bit.  ``clips``
(a dict) counts the values each of the four clips changed: "channel", "q", "r",
"app".
"""
import numpy as np

from ldpc_layered_ref import Layers, code_layers, truncated, var_of  # noqa: F401  (reused, re-exported)

DEFAULT = (2, 6, 8)  # frac_bits, msg_bits, app_bits


def parameters(frac_bits, msg_bits, app_bits, corr_factor):
    """(rmax, amax, alpha); ValueError outside the library's ranges."""
    for name, x in (("frac_bits", frac_bits), ("msg_bits", msg_bits), ("app_bits", app_bits)):
        if int(x) != x:
            raise ValueError(f"{name} must be an integer")
    if not 0 <= frac_bits <= 8:
        raise ValueError("frac_bits must lie in 0..8")
    if not 2 <= msg_bits <= 8:
        raise ValueError("msg_bits must lie in 2..8")
    if not msg_bits <= app_bits <= 16:
        raise ValueError("app_bits must lie in msg_bits..16")
    a = np.rint(16.0 * np.float64(corr_factor))
    if not 1 <= a <= 16:  # (a NaN fails both)
        raise ValueError("rint(16 corr_factor) must lie in 1..16")
    return (1 << (int(msg_bits) - 1)) - 1, (1 << (int(app_bits) - 1)) - 1, int(a)


def _count(clips, key, before, after):
    if clips is not None:
        clips[key] = clips.get(key, 0) + int(np.count_nonzero(before != after))


def quantise(ch, frac_bits, rmax, clips=None):
    """The channel LLRs as integers: rint (half to even) of ch 2^F, clipped to
    +-rmax; NaN -> 0; +-inf and +-DBL_MAX saturate; -0.0 -> 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.rint(np.asarray(ch, np.float64) * float(1 << frac_bits))
    x = np.where(np.isnan(x), 0.0, x)
    y = np.clip(x, -rmax, rmax)
    _count(clips, "channel", x, y)
    return y.astype(np.int64)


def scale(alpha, m, rmax):
    """min((alpha m + 8) >> 4, rmax)"""
    return np.minimum((alpha * np.asarray(m, np.int64) + 8) >> 4, rmax)


def check_rule(Q, alpha, rmax, amax, clips=None):
    """The new r of the checks whose q are the rows of Q (n, dc).  The minimum
    over a check's other edges is its second smallest |q| where |q[e]| is the
    smallest and the smallest elsewhere; with the two smallest equal both
    readings of "the" smallest give the same values."""
    A = np.abs(Q)
    S = np.sort(A, axis=1)
    m1 = S[:, :1]
    m2 = S[:, 1:2] if Q.shape[1] > 1 else np.full_like(m1, amax)
    mag = np.where(A == m1, m2, m1)
    neg = Q < 0
    neg_others = np.logical_xor.reduce(neg, axis=1)[:, None] ^ neg
    m = scale(alpha, mag, rmax)
    _count(clips, "r", (alpha * mag + 8) >> 4, m)
    return np.where(neg_others, -m, m)


def decode(ch, vdeg, cdeg, intrlv, first_check, frac_bits=2, msg_bits=6, app_bits=8, corr_factor=0.75, max_it=200,
           order="layer", trace=False, layers=None, clips=None):
    """(app, it): app = int 2^-F as float64 (a zero is +0), it as
    ldpc_layered_ref.decode.  trace=True returns (app, it, apps): app at every
    stop test made (apps[i]: after i sweeps), with the final app appended when
    the word ran out; ``truncated`` cuts such a run (not at 0: max_it = 0
    returns ch itself)."""
    rmax, amax, alpha = parameters(frac_bits, msg_bits, app_bits, corr_factor)
    assert order in ("layer", "check")
    if max_it == 0:
        ch = np.array(ch, dtype=np.float64)
        return (ch, 0, ch[None, :].copy()) if trace else (ch, 0)
    g = layers or Layers(vdeg, cdeg, intrlv, first_check)
    down = 1.0 / (1 << frac_bits)
    app = quantise(ch, frac_bits, rmax, clips)
    r = np.zeros(len(g.var_of), dtype=np.int64)
    apps = []

    def out(it):
        a = app * down
        if not trace:
            return a, it
        if it == max_it:
            apps.append(a)
        return a, it, np.array(apps).reshape(len(apps), len(app))

    for it in range(max_it):
        if trace:
            apps.append(app * down)
        if g.stop(app):
            return out(it)
        for by_deg in g.groups:
            for E, V in by_deg:
                rows = [slice(None)] if order == "layer" else [slice(i, i + 1) for i in range(len(E))]
                for s in rows:
                    d = app[V[s]] - r[E[s]]
                    q = np.clip(d, -amax, amax)
                    _count(clips, "q", d, q)
                    rn = check_rule(q, alpha, rmax, amax, clips)
                    r[E[s]] = rn
                    t = q + rn
                    a = np.clip(t, -amax, amax)
                    _count(clips, "app", t, a)
                    app[V[s]] = a
    return out(max_it)


def decode_code(c, ch, widths=DEFAULT, **kw):
    return decode(ch, c.vdeg, c.cdeg, c.intrlv, code_layers(c), *widths, **kw)
