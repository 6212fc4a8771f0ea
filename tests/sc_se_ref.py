"""NumPy statement of state evolution for spatially coupled SPARCs (no tests
here): what sa_sc_se (csrc/sa_se.hip) is held to.  Test
infrastructure only: the product never imports this module.

For one configuration: an allocation Pl (L,), section size M, code length n,
an R x C base matrix W, noise sigma and S rows U[s] of M standard Gaussians
(column 0 is the true column).  With c_l = sqrt(n Pl_l), column block
c(l) = l // (L // C) and P_c = sum_{l in c} Pl_l (l in order):

    psi_c^0 = P_c
    phi_r^t    = sigma^2 + sum_c W[r, c] psi_c^t                 (c in order)
    1/tau_c^2  = (1 / R) sum_r W[r, c] / phi_r^t                 (r in order)
    a          = c_l / tau_c(l)
    E_l        = mean_s softmax(a^2 + a U[s, 0], a U[s, 1:])[0]  (se_ref.posterior)
    x_c^t      = sum_{l in c} (Pl_l / P_c) E_l
    psi_c^{t+1} = P_c (1 - x_c^t)
    (l, s) is missed at t when a^2 + a U[s, 0] < max_{j >= 1} a U[s, j].

The predicted stop index is the first t >= 1 at which every phi_r^t equals
phi_r^{t-1} bit for bit, or T.  It works section by section, with no classes
and no skipping, in binary64 or (longdouble=True) in np.longdouble."""
import numpy as np

from se_ref import posterior


def block_powers(Pl, C):
    """P_c: the powers of each column block added in section order."""
    Pl = np.asarray(Pl)
    return np.array([np.cumsum(blk)[-1] for blk in Pl.reshape(C, -1)], dtype=Pl.dtype)


def phi_tau(W, sig2, psi):
    """phi_r = sig2 + sum_c W[r, c] psi_c and tau_c^2 = 1 / ((sum_r W[r, c] / phi_r) / R),
    each sum in index order from 0."""
    R, C = W.shape
    ft = psi.dtype.type
    phi = np.zeros(R, dtype=psi.dtype)
    tau2 = np.zeros(C, dtype=psi.dtype)
    for r in range(R):
        acc = ft(0)
        for c in range(C):
            acc = acc + W[r, c] * psi[c]
        phi[r] = sig2 + acc
    for c in range(C):
        acc = ft(0)
        for r in range(R):
            acc = acc + W[r, c] / phi[r]
        tau2[c] = ft(1) / (acc / ft(R))
    return phi, tau2


def sc_se_ref(Pl, sigma, M, n, W, T, U, longdouble=False, margin=False):
    """One configuration.  Returns phi (T+1, R), tau2 (T, C), x (T, C), miss
    (T, C) int64, E (L,) of the last iteration and the predicted stop index;
    with ``margin`` also the smallest relative margin
    |l0 - mo| / max(|l0|, |mo|) of any miss comparison."""
    ft = np.longdouble if longdouble else np.float64
    Pl = np.asarray(Pl, dtype=np.float64).astype(ft).reshape(-1)
    W = np.asarray(W, dtype=np.float64).astype(ft)
    U = np.asarray(U, dtype=np.float64).astype(ft)
    L, (R, C), S = Pl.size, W.shape, U.shape[0]
    assert U.shape == (S, M) and M >= 2 and n % R == 0 and L % C == 0
    Lc = L // C
    sig2 = ft(sigma) * ft(sigma)
    c_l = np.sqrt(ft(n) * Pl)
    Pc = block_powers(Pl, C)
    phi = np.zeros((T + 1, R), dtype=ft)
    tau2 = np.zeros((T, C), dtype=ft)
    x = np.zeros((T, C), dtype=ft)
    miss = np.zeros((T, C), dtype=np.int64)
    E = np.zeros(L, dtype=ft)
    worst = np.inf
    psi = Pc.copy()
    stop = T
    for t in range(T + 1):
        phi[t], tau2_t = phi_tau(W, sig2, psi)
        if t >= 1 and stop == T and np.array_equal(phi[t], phi[t - 1]):
            stop = t
        if t == T:
            break
        tau2[t] = tau2_t
        tau = np.sqrt(tau2_t)
        for l in range(L):
            c = l // Lc
            post, l0, mo = posterior(c_l[l] / tau[c], U)
            E[l] = post.sum() / ft(S)
            miss[t, c] += int((l0 < mo).sum())
            if margin:
                den = np.maximum(np.abs(l0), np.abs(mo))
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = min(worst, float(np.min(np.where(den > 0, np.abs(l0 - mo) / den, 0.0))))
        for c in range(C):
            sl = slice(c * Lc, (c + 1) * Lc)
            x[t, c] = (Pl[sl] / Pc[c] * E[sl]).sum()
        psi = Pc * (ft(1) - x[t])
    return (phi, tau2, x, miss, E, stop, worst) if margin else (phi, tau2, x, miss, E, stop)
