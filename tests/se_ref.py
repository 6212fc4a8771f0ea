"""NumPy statement of the AMP decoder's finite-M state evolution (no tests
here): what sa_se (csrc/sa_se.hip) is held to.  Test infrastructure only: the
product never imports this module.

For an allocation Pl (P = sum Pl), section size M, code length n, noise sigma
and S rows U[s] of M standard Gaussians (column 0 is the true column):

    tau_0^2 = sigma^2 + P,   c_l = sqrt(n Pl_l),   a = c_l / tau_t,
    logits of (l, s):  a^2 + a U[s, 0]  and  a U[s, j], j >= 1,
    E_l = mean_s softmax(logits)[0],
    x_{t+1} = sum_l (Pl_l / P) E_l,   tau_{t+1}^2 = sigma^2 + P (1 - x_{t+1}),
    (l, s) is missed at t when a^2 + a U[s, 0] < max_{j >= 1} a U[s, j].

It works section by section, with no grouping of equal powers, in binary64 or
(longdouble=True) in np.longdouble."""
import numpy as np


def posterior(a, U):
    """Per row of U (S, M): the posterior of column 0, its logit and the
    largest other logit, for the scalar a = c / tau."""
    l0 = a * a + a * U[:, 0]
    lo = a * U[:, 1:]
    mo = lo.max(axis=1)
    mx = np.maximum(l0, mo)
    e0 = np.exp(l0 - mx)
    es = np.exp(lo - mx[:, None]).sum(axis=1)
    return e0 / (e0 + es), l0, mo


def se_ref(Pl, sigma, M, n, T, U, longdouble=False, margin=False):
    """Pl (B, L), sigma a scalar or (B,), U (S, M).  Returns tau2 (B, T+1),
    x (B, T), miss (B, T) int64 and E (B, L) of the last iteration; with
    ``margin`` also the smallest relative margin |l0 - mo| / max(|l0|, |mo|)
    of any miss comparison."""
    ft = np.longdouble if longdouble else np.float64
    Pl = np.atleast_2d(np.asarray(Pl, dtype=np.float64)).astype(ft)
    B, L = Pl.shape
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,)).astype(ft)
    U = np.asarray(U, dtype=np.float64).astype(ft)
    S = U.shape[0]
    assert U.shape == (S, M) and M >= 2
    tau2 = np.zeros((B, T + 1), dtype=ft)
    x = np.zeros((B, T), dtype=ft)
    miss = np.zeros((B, T), dtype=np.int64)
    E = np.zeros((B, L), dtype=ft)
    worst = np.inf
    for b in range(B):
        P = Pl[b].sum()
        c = np.sqrt(ft(n) * Pl[b])
        tau2[b, 0] = sig[b] * sig[b] + P
        for t in range(T):
            tau = np.sqrt(tau2[b, t])
            for l in range(L):
                post, l0, mo = posterior(c[l] / tau, U)
                E[b, l] = post.sum() / ft(S)
                miss[b, t] += int((l0 < mo).sum())
                if margin:
                    den = np.maximum(np.abs(l0), np.abs(mo))
                    with np.errstate(invalid="ignore", divide="ignore"):
                        worst = min(worst, float(np.min(np.where(den > 0, np.abs(l0 - mo) / den, 0.0))))
            x[b, t] = (Pl[b] / P * E[b]).sum()
            tau2[b, t + 1] = sig[b] * sig[b] + P * (ft(1) - x[b, t])
    return (tau2, x, miss, E, worst) if margin else (tau2, x, miss, E)
