"""The NumPy statement of coupled AMP from a beta_0 and of the joint coupled
SPARC + LDPC decoder: what sa_sc_amp_start, the staged
coupled context and sc_joint.CoupledJointDecoder are held to.

amp_sc_start is sc_wave_ref.amp_sc_wave's loop (which at tolerances 0 is
sc_ref.amp_sc's) with the reference's start (sparc_ldpc.py:192-200) on the
coupled design: beta <- beta_0 and z <- y - A beta_0, no Onsager term; iteration
0's step 4 reads beta = beta_0.  With beta0 None, beta = 0 and z = y.

joint_rep is one rep of the `soft` (soft_amp_ldpc_sim, sparc_ldpc.py:547-712) or
`hard` (hardinitbeta_amp_ldpc_sim, :715-860) exchange on a coupled design, built
from the oracles alone: oracle.glue_oracle (llr, soft_beta0, hard_indices,
onehot) and oracle.ldpc_oracle (protograph, prepare_decoder, encode, sumprod2's
decoder with its trace), drawn in joint.draw_reps' order.
"""
import numpy as np

from oracle import glue_oracle as go
from oracle import ldpc_oracle as lo


def amp_sc_start(y, Pl, W, L, M, T, A, beta0=None, stop_tol=0.0, freeze_tol=0.0, early_stop=True, dtype=np.float64):
    """-> (beta (L*M,), stop index (T: ran out), phi (T, R), live (T, C) uint8,
    snaps {t: beta after t iterations}, margin): sc_wave_ref.amp_sc_wave's
    results, from the start beta0 (L*M,) (None: zero)."""
    dt = np.dtype(dtype).type
    W = np.asarray(W, dtype=dt)
    R, C = W.shape
    y = np.asarray(y, dtype=dt).reshape(-1)
    Pl = np.asarray(Pl, dtype=dt)
    A = np.asarray(A, dtype=dt)
    stol, ftol = dt(stop_tol), dt(freeze_tol)
    n = y.size
    nr, Lc = n // R, L // C
    rb = np.arange(n) // nr
    cbj = (np.arange(L) // Lc).repeat(M)
    cl = np.sqrt(dt(n) * Pl)
    cj = cl.repeat(M)
    Pc = Pl.reshape(C, Lc).sum(axis=1)
    if beta0 is None:
        beta = np.zeros(L * M, dtype=dt)
        z = y.copy()
    else:
        beta = np.asarray(beta0, dtype=dt).reshape(-1).copy()                # the start
        assert beta.size == L * M
        z = y - A @ beta
    phi_tr = np.zeros((T, R), dtype=dt)
    live_tr = np.zeros((T, C), dtype=np.uint8)
    snaps = {0: beta.copy()}
    last = None
    taul = None
    stop = T
    margin = np.inf

    def note(ratio, tol):
        nonlocal margin
        m = np.abs(np.asarray(ratio, dtype=np.float64) - float(tol)) / float(tol)
        margin = min(margin, float(m.min()))

    for t in range(T):
        phi = (z ** 2).reshape(R, nr).sum(axis=1) / dt(nr)                 # step 1
        if early_stop and t > 0:                                           # step 2'
            if stol > 0:
                note(np.abs(phi.astype(np.float64) - last) / last.astype(np.float64), stol)
            if np.all(np.abs(phi - last) <= stol * last):
                stop = t
                break
        last = phi
        phi_tr[t] = phi
        s = (W / phi[:, None]).sum(axis=0)                                 # step 3'
        inv_tau2 = s / dt(R)
        tau2 = dt(R) / s
        if t == 0 or not ftol > 0:
            live = np.ones(C, dtype=bool)
        else:
            note(np.abs(tau2.astype(np.float64) - taul) / taul.astype(np.float64), ftol)
            live = np.abs(tau2 - taul) > ftol * taul
        taul = tau2.copy() if taul is None else np.where(live, tau2, taul)
        live_tr[t] = live
        u = beta * cj * inv_tau2[cbj] + cj * (A.T @ (z / phi[rb]))         # step 4
        u = u.reshape(L, M)
        e = np.exp(u - u.max(axis=1, keepdims=True))                       # step 5 (per-section max)
        new = (cl[:, None] * e / e.sum(axis=1, keepdims=True)).reshape(-1)
        beta = np.where(live[cbj], new, beta)                              # live blocks only
        psi = Pc - (beta ** 2).reshape(C, Lc * M).sum(axis=1) / dt(n)      # step 6
        gamma = W @ psi
        z = y - A @ beta + z * gamma[rb] / phi[rb]                         # step 7
        snaps[t + 1] = beta.copy()
    return beta, stop, phi_tr, live_tr, snaps, margin


class Graph:
    """An LDPC code for joint_rep: the protograph and the decoder's graph."""

    def __init__(self, standard="802.16", rate="5/6", z=8):
        self.standard, self.rate, self.z = standard, rate, z
        self.proto = lo.protograph(standard, rate, z)
        self.vdeg, self.cdeg, self.intrlv = lo.prepare_decoder(self.proto, z)
        self.N = self.proto.shape[1] * z
        self.K = self.N - self.proto.shape[0] * z

    def encode(self, info):
        return lo.encode(self.proto, self.z, info)

    def decode(self, ch, max_it=lo.MAX_ITCOUNT):
        """sumprod2 with its trace: (app, it, smallest stop margin over the iterations run)."""
        app, it, _, margins = lo._decode(ch, self.vdeg, self.cdeg, self.intrlv, "sumprod2", max_it=max_it, trace=True)
        return app.copy(), int(it), float(np.min(margins)) if len(margins) else np.inf


def draw(graph, L, M, n, rs, sigma):
    """One rep in joint.draw_reps' order: the protected bits, the unprotected
    bits, the noise; message = unprotected bits then the LDPC codeword, MSB
    first per section.  -> (section indices (L,), noise (n,))."""
    lgm = int(M).bit_length() - 1
    prot = rs.randint(0, 2, graph.K)
    unprot = rs.randint(0, 2, L * lgm - graph.N)
    noise = rs.randn(n, 1).reshape(-1) * sigma
    bits = np.concatenate([unprot, graph.encode(prot)]).reshape(L, lgm)
    return (bits << np.arange(lgm - 1, -1, -1)).sum(axis=1).astype(np.int64), noise


def bit_errors(a, b):
    x = np.bitwise_xor(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    return int(sum(bin(int(v)).count("1") for v in x.reshape(-1)))


def top_two_gap(beta, cl, L, M):
    """Smallest (largest - second largest) / c_l over the sections: how far the nearest decision is from a tie."""
    s = np.sort(np.asarray(beta, dtype=np.float64).reshape(L, M), axis=1)
    return float(((s[:, -1] - s[:, -2]) / cl).min())


def joint_rep(case, graph, seed, mode, soft_iter=2, T=30, rs=None, sigma=None, max_it=lo.MAX_ITCOUNT):
    """One rep of RandomState(seed) (or of the generator rs) on the coupled
    case.  -> dict: idx, noise, y; betas and stops (the estimate and the stop
    index of every AMP call), llrs, apps, decs (the decisions after every BP call, (L,)), amp / ldpc /
    bp_iters (the counts JointDecoder.run returns for the rep), bp_margin (the
    smallest stop margin of any BP call) and gap (the smallest top-two gap of
    any estimate)."""
    assert mode in ("soft", "hard")
    L, M, n, Pl, W, A = case.L, case.M, case.n, case.Pl, case.W, case.A
    lgm = int(M).bit_length() - 1
    ns = graph.N // lgm
    l0 = L - ns
    assert graph.N % lgm == 0 and l0 >= 0
    rs = np.random.RandomState(seed) if rs is None else rs
    idx, noise = draw(graph, L, M, n, rs, case.sigma if sigma is None else sigma)
    cl = np.sqrt(n * np.asarray(Pl, dtype=np.float64))
    y = A @ _onehot(idx, cl, M) + noise
    out = dict(idx=idx, noise=noise, y=y, betas=[], stops=[], llrs=[], apps=[], decs=[], amp=[], ldpc=[], bp_iters=[],
               bp_margin=np.inf, gap=np.inf)

    def amp_call(beta0):
        beta, stop = amp_sc_start(y, Pl, W, L, M, T, A, beta0=beta0)[:2]
        out["betas"].append(beta)
        out["stops"].append(stop)
        out["gap"] = min(out["gap"], top_two_gap(beta, cl, L, M))
        rx = beta.reshape(L, M).argmax(axis=1)
        out["amp"].append(bit_errors(rx, idx))
        return beta, rx

    def bp_call(beta, rx):
        llr = np.asarray(go.llr(beta[None, :], n, Pl, L, M, l0, ns)[0], dtype=np.float64)[0]
        app, it, margin = graph.decode(llr, max_it)
        dec = rx.copy()
        dec[l0:] = go.hard_indices(app[None, :], M)[0]
        out["llrs"].append(llr)
        out["apps"].append(app)
        out["decs"].append(dec)
        out["bp_iters"].append(it)
        out["ldpc"].append(bit_errors(dec, idx))
        out["bp_margin"] = min(out["bp_margin"], margin) if margin == margin else 0.0  # NaN: no margin
        return app, dec

    beta, rx = amp_call(None)
    if mode == "soft":
        for _ in range(soft_iter):
            app, _ = bp_call(beta, rx)
            b0 = np.asarray(go.soft_beta0(beta[None, :], app[None, :], n, Pl, L, M, l0, ns), dtype=np.float64)[0]
            beta, rx = amp_call(b0)
    else:
        _, dec = bp_call(beta, rx)
        b0 = np.asarray(go.onehot(n, Pl, M, dec[None, :]), dtype=np.float64)[0]
        beta, rx = amp_call(b0)
    return out


def _onehot(idx, cl, M):
    L = len(idx)
    b = np.zeros(L * M)
    b[np.arange(L) * M + np.asarray(idx)] = cl
    return b
