"""The NumPy statement of base-matrix AMP for spatially coupled SPARCs (DESIGN.md
section 13), over the oracle's dense design matrix: the reference the device
decoder (sa_sc_*, k_scsec / k_scrow) is held to.  Binary64 throughout.

Coupled design: A[i, j] = sqrt(W[r(i), c(j)]) * At[i, j], At =
oracle.amp_oracle.dense_design_matrix (entries +-1/sqrt(n)), row block
r(i) = i // (n // R), column block c(l) = l // (L // C).
"""
import numpy as np

from oracle import amp_oracle as orc


def base_matrix(omega, Lambda):
    """W[r, c] = R / omega for c <= r <= c + omega - 1, R = Lambda + omega - 1, C = Lambda."""
    R = Lambda + omega - 1
    W = np.zeros((R, Lambda))
    for c in range(Lambda):
        W[c:c + omega, c] = R / omega
    return W


def coupled_matrix(L, M, n, W, ordering):
    """The dense coupled design, n x (L*M)."""
    W = np.asarray(W, dtype=np.float64)
    R, C = W.shape
    assert n % R == 0 and L % C == 0
    rb = np.arange(n) // (n // R)
    cb = (np.arange(L) // (L // C)).repeat(M)
    return orc.dense_design_matrix(L, M, n, ordering) * np.sqrt(W[rb][:, cb])


def amp_sc(y, Pl, W, L, M, T, A, early_stop=True):
    """The loop.  -> (beta (L*M,), stop index (T: ran out), phi (T, R) with the
    rows from the stop index on zero, snaps {t: beta after t iterations})."""
    W = np.asarray(W, dtype=np.float64)
    R, C = W.shape
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    Pl = np.asarray(Pl, dtype=np.float64)
    n = y.size
    nr, Lc = n // R, L // C
    rb = np.arange(n) // nr
    cbj = (np.arange(L) // Lc).repeat(M)
    cl = np.sqrt(n * Pl)
    cj = cl.repeat(M)
    Pc = Pl.reshape(C, Lc).sum(axis=1)
    beta = np.zeros(L * M)
    z = y.copy()
    phi_tr = np.zeros((T, R))
    snaps = {0: beta.copy()}
    last = None
    stop = T
    for t in range(T):
        phi = (z ** 2).reshape(R, nr).sum(axis=1) / nr                    # step 1
        if early_stop and t > 0 and np.array_equal(phi, last):            # step 2
            stop = t
            break
        last = phi
        phi_tr[t] = phi
        inv_tau2 = (W / phi[:, None]).sum(axis=0) / R                     # step 3
        u = beta * cj * inv_tau2[cbj] + cj * (A.T @ (z / phi[rb]))        # step 4
        u = u.reshape(L, M)
        e = np.exp(u - u.max(axis=1, keepdims=True))                      # step 5 (per-section max)
        beta = (cl[:, None] * e / e.sum(axis=1, keepdims=True)).reshape(-1)
        psi = Pc - (beta ** 2).reshape(C, Lc * M).sum(axis=1) / n         # step 6
        gamma = W @ psi
        z = y - A @ beta + z * gamma[rb] / phi[rb]                        # step 7
        snaps[t + 1] = beta.copy()
    return beta, stop, phi_tr, snaps


def rep(L, M, n, Pl, sigma, A, seed):
    """The project's synthetic rep on the coupled design: RandomState(seed)
    draws the section indices, then the noise.  -> (idx, y)"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, M, L)
    beta0 = np.zeros(L * M)
    beta0[np.arange(L) * M + idx] = np.sqrt(n * np.asarray(Pl))
    y = A @ beta0 + rs.randn(n) * sigma
    return idx, y
