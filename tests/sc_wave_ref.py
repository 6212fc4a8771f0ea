"""The NumPy statement of the coupled decoder's opt-in tolerance stop and frozen
column blocks, over sc_ref's dense coupled matrix: what
sa_sc_amp_ex / sa_sc_mc_ex (the wave form of k_scsec) are held to.

The loop is sc_ref.amp_sc's with two real parameters and one state vector,
in the working precision `dtype` (np.float32 / np.float64):

  2'. at t > 0 stop with index t if for every r
      |phi_r - phi_r^(t-1)| <= stop_tol * phi_r^(t-1)      (stop_tol = 0: bit equality)
  3'. tau_c^2 = R / sum_r W[r, c] / phi_r (r in order); block c is live at t if
      t = 0, or freeze_tol == 0, or |tau_c^2 - taul_c| > freeze_tol * taul_c;
      for live blocks taul_c <- tau_c^2
  4-5 for live blocks only: a frozen block's beta stays (and with it its psi_c
      and its A beta); 6-7 unchanged.  Nothing is sticky: a frozen block is live
      again whenever its tau_c^2 has drifted from taul_c.

The margin of a run is the smallest |ratio - tol| / tol over every comparison
it made (ratio = |phi_r - last_r| / last_r against stop_tol, |tau_c^2 - taul_c|
/ taul_c against freeze_tol; formed in binary64 from the working-precision
values): how far the nearest decision was from flipping.
"""
import numpy as np


def amp_sc_wave(y, Pl, W, L, M, T, A, stop_tol=0.0, freeze_tol=0.0, early_stop=True, dtype=np.float64):
    """-> (beta (L*M,), stop index (T: ran out), phi (T, R), live (T, C) uint8,
    snaps {t: beta after t iterations}, margin (inf: no comparison made)).
    Rows of phi and live from the stop index on are zero."""
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
    beta = np.zeros(L * M, dtype=dt)
    z = y.copy()
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


def frozen_count(live, stop):
    """Frozen block-iterations before the stop index, and the block-iterations there were."""
    live = np.asarray(live)[:stop]
    return int(live.size - live.sum()), int(live.size)


def unfreeze_events(live, stop):
    """How often a block that was frozen at t - 1 is live at t, before the stop index."""
    live = np.asarray(live)[:stop].astype(bool)
    return int((~live[:-1] & live[1:]).sum()) if stop > 1 else 0
