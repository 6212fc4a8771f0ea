"""The layered (row-layered, turbo-decoding message passing) belief-propagation
schedule in NumPy: the parity target of the HIP kernel k_bpl.
Test infrastructure only: the product never imports this module.

    app = ch;  r = 0
    for it in 0 .. max_iter-1:
        if stop(app): return app, it
        for each layer, in order:
            for each check c of the layer, each of its edges e in port order (v = var_of[e]):
                q[e] = app[v] - r[e]
            r[edges of c] = check rule on q[edges of c]
            app[v] = q[e] + r[e]
    return app, max_iter

The check rule is the flooding decoders' own (oracle.ldpc_oracle.lxfb): Lxfb
with the correction terms ("sumprod2"), or Lxfb without them and the outputs
times corr_factor ("minsum").  stop(app): every check has an even number of
variables with app < 0 and none with app == 0 or NaN (an erased bit leaves its
checks unsatisfied, as the flooding rule b[0] > 0 does).  Layer l is the
consecutive checks first_check[l] .. first_check[l+1]-1; no variable may occur
twice in a layer, so the checks of a layer are independent and every order of
processing them gives the same bits.  Two orders are offered and must agree
bit for bit: one check at a time (order="check") and one layer at a time,
vectorised over its checks of equal degree (order="layer").
"""
import numpy as np

from oracle import ldpc_oracle as lo

ALGOS = ("sumprod2", "minsum")


def lxor_log1p(L1, L2, corr=True):
    """lo.lxor with log1p(x) for log(1 + x): the perturbation of Lxor's
    logarithm that the knife-edge precondition of the GPU tests is taken from."""
    s = np.where(np.signbit(L1) == np.signbit(L2), 1.0, -1.0)
    L = s * np.fmin(np.abs(L1), np.abs(L2))
    if corr:
        with np.errstate(over="ignore", invalid="ignore"):
            L = L + np.log1p(np.exp(-np.abs(L1 + L2)))
            L = L - np.log1p(np.exp(-np.abs(L1 - L2)))
    return L


def _lxfb_with(Lm, corr, lxor):
    """lo.lxfb with another Lxor (same loop structure, same operand order)."""
    dc = Lm.shape[1]
    f = [None] * dc
    b = [None] * dc
    f[0] = Lm[:, 0].copy()
    b[dc - 1] = Lm[:, dc - 1].copy()
    for k in range(1, dc):
        f[k] = lxor(f[k - 1], Lm[:, k], corr)
        b[dc - k - 1] = lxor(b[dc - k], Lm[:, dc - k - 1], corr)
    Lm[:, 0] = b[1]
    Lm[:, dc - 1] = f[dc - 2]
    for k in range(1, dc - 1):
        Lm[:, k] = lxor(f[k - 1], b[k + 1], corr)
    return b[0]


def var_of(vdeg, intrlv):
    """var_of[e]: the variable node of edge e (messages in check order)."""
    vdeg = np.asarray(vdeg, np.int64)
    out = np.empty(len(intrlv), dtype=np.int64)
    out[np.asarray(intrlv, np.int64)] = np.repeat(np.arange(len(vdeg)), vdeg)
    return out


def protograph_layers(Nc, z):
    """The layers of a quasi-cyclic code: its protograph rows."""
    return np.arange(0, Nc + 1, z, dtype=np.int64)


class Layers:
    """The graph in the layout the schedule walks: cstart[Nc + 1], var_of[Nmsg],
    first_check[nlayers + 1].  Asserts that the layering is one."""

    def __init__(self, vdeg, cdeg, intrlv, first_check):
        self.cdeg = np.asarray(cdeg, np.int64)
        self.cstart = np.concatenate([[0], np.cumsum(self.cdeg)])
        self.var_of = var_of(vdeg, intrlv)
        self.Nv, self.Nc = len(vdeg), len(self.cdeg)
        fc = np.asarray(first_check, np.int64)
        assert len(fc) >= 2 and fc[0] == 0 and fc[-1] == self.Nc and np.all(np.diff(fc) > 0), \
            "first_check must increase strictly from 0 to Nc"
        self.first_check = fc
        self.groups = []  # per layer: [(edge matrix (n, dc), variables (n, dc)) per check degree]
        for l in range(len(fc) - 1):
            e0, e1 = self.cstart[fc[l]], self.cstart[fc[l + 1]]
            v, n = np.unique(self.var_of[e0:e1], return_counts=True)
            assert np.all(n == 1), f"layer {l}: variable {int(v[np.argmax(n > 1)])} occurs twice"
            checks = np.arange(fc[l], fc[l + 1])
            by_deg = []
            for d in np.unique(self.cdeg[checks]):
                cs = checks[self.cdeg[checks] == d]
                E = self.cstart[cs][:, None] + np.arange(d)[None, :]
                by_deg.append((E, self.var_of[E]))
            self.groups.append(by_deg)

    def stop(self, app):
        neg = (app < 0)[self.var_of].astype(np.int64)
        with np.errstate(invalid="ignore"):
            undecided = (~((app > 0) | (app < 0)))[self.var_of].astype(np.int64)
        odd = np.add.reduceat(neg, self.cstart[:-1]) & 1
        return not (odd.any() or np.add.reduceat(undecided, self.cstart[:-1]).any())


def decode(ch, vdeg, cdeg, intrlv, first_check, algo="sumprod2", corr_factor=0.7, max_it=lo.MAX_ITCOUNT,
           order="layer", trace=False, log1p=False, layers=None):
    """(app, it): it = i means the stop test passed after i sweeps (0: the
    channel word is a codeword already); max_it: it had not passed before the
    last sweep.  max_it = 0 gives (ch, 0).

    trace=True returns (app, it, apps, margins): app and the smallest non-zero
    |app| at every stop test made (apps[i]: after i sweeps), with the word's
    final app appended when it ran out.  ``truncated`` cuts such a run."""
    if algo not in ALGOS:
        raise NameError("Decoder type unknonwn")
    assert order in ("layer", "check")
    g = layers or Layers(vdeg, cdeg, intrlv, first_check)
    corr = algo == "sumprod2"

    def rule(Lm):
        if log1p:
            _lxfb_with(Lm, corr, lxor_log1p)
        else:
            lo.lxfb(Lm, corr)
        return Lm if corr else Lm * corr_factor

    app = np.array(ch, dtype=np.float64)
    r = np.zeros(len(g.var_of))
    apps, margins = [], []

    def out(it):
        if not trace:
            return app, it
        if it == max_it:
            apps.append(app.copy())
        return app, it, np.array(apps).reshape(len(apps), len(app)), np.array(margins)

    with np.errstate(over="ignore", invalid="ignore"):
        for it in range(max_it):
            if trace:
                apps.append(app.copy())
                nz = np.abs(app[app != 0])
                margins.append(nz.min() if len(nz) else np.inf)
            if g.stop(app):
                return out(it)
            for by_deg in g.groups:
                for E, V in by_deg:
                    rows = [slice(None)] if order == "layer" else [slice(i, i + 1) for i in range(len(E))]
                    for s in rows:
                        q = app[V[s]] - r[E[s]]
                        rn = rule(q.copy())
                        r[E[s]] = rn
                        app[V[s]] = q + rn
    return out(max_it)


def truncated(it, apps, k):
    """(app, it) of the decode cut at max_it = k <= the traced run's max_it."""
    if k > it:  # the traced run stopped after ``it`` sweeps
        return apps[it], it
    return apps[k], k


def code_layers(c):
    return protograph_layers(c.Nc, c.z)


def decode_code(c, ch, algo="sumprod2", **kw):
    return decode(ch, c.vdeg, c.cdeg, c.intrlv, code_layers(c), algo, **kw)
