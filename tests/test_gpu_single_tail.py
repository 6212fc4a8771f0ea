"""The single-codeword decode's row launches and fixed launches: the
per-codeword power read with a row launch's first loads, the iters writes
carried by the row launches, the estimate's final buffer chosen on the host,
no zero fill of the first iteration's previous estimate, and the decisions
written by the kernel into the pinned ring.  Small shapes; the oracle is
oracle.amp_oracle (the reference's loop in binary64 NumPy)."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import amp_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-5, "fp64": 1e-11}


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_ORACLE = {}


def oracle_ops(L, M, n):
    """The oracle's (Ab, Az) of a shape, built once for the module."""
    if (L, M, n) not in _ORACLE:
        _ORACLE[(L, M, n)] = orc.sparc_transforms(L, M, n)[:2]
    return _ORACLE[(L, M, n)]


def reps(L, M, n, Pls, sigma, seed0):
    """One rep per row of Pls (B, L): y (B, n), each with its own allocation."""
    Ab, _ = oracle_ops(L, M, n)
    return np.stack([orc.rep_inputs(L, M, n, Pls[b], sigma, Ab, seed0 + b)[1].reshape(-1)
                     for b in range(len(Pls))])


def decode(op, ys, Pl, T, early_stop=False, beta0=None):
    """Stage and run on `op`; (beta, iters) of the staged batch."""
    B = ys.shape[0]
    op.stage(ys, Pl, beta0)
    op.run(B, T, early_stop=early_stop, beta0=beta0 is not None)
    op.wait()
    return op.fetch(B)


# ---- 1. per-codeword power through every row kernel -------------------------

POWER_CASES = [
    # L, M, n, B, plan, row kernel
    (64, 512, 576, 3, None, "k_row2"),
    (64, 512, 581, 3, None, "k_row2"),        # n no multiple of 16: a partial last row block
    (64, 512, 576, 3, "NO_ROW16", "k_row2"),
    (64, 512, 581, 3, "NO_ROW16", "k_row2"),
    (64, 512, 576, 1, None, None),            # one codeword: 16-row blocks in binary32
    (64, 64, 384, 5, None, "k_rowc"),         # the batched row kernel
]


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("L,M,n,B,plan,row", POWER_CASES)
def test_per_codeword_power_vs_oracle(sp, prec, L, M, n, B, plan, row):
    """sa_stage_power_batch with a different total power P_b per codeword: the
    Onsager term of codeword b (sparc_ldpc.py:220) uses P_b, which the row
    kernels now load with their first loads.  Codeword by codeword against the
    oracle after 1, 2 and 5 iterations; a wrong b * Pbst index takes another
    codeword's P and misses TOL at t = 2 already."""
    op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=prec,
                          plan=None if plan is None else (plan,))
    if row is not None:
        assert op.plan(B)["row_kernel"] == row, op.plan(B)
    else:
        assert op.plan(B)["row_kernel"] == ("k_row2_16" if prec == "fp32" else "k_row2"), op.plan(B)
    Ptot = 1.5 + 0.75 * np.arange(B)  # 1.5, 2.25, 3.0, ...
    Pls = Ptot[:, None] / L * np.ones((B, L))
    ys = reps(L, M, n, Pls, 0.6, 300)
    Ab, Az = oracle_ops(L, M, n)
    op.reserve(B, 5)
    op.stage(ys, Pls[0])
    op.stage_power_batch(B, Pls)
    for T in (1, 2, 5):
        op.run(B, T, early_stop=False)
        op.wait()
        bb, it = op.fetch(B)
        assert np.array_equal(it, np.full(B, T))
        for b in range(B):
            ref = orc._amp_core(ys[b].reshape(-1, 1), Pls[b], L, M, T, Ab, Az, None, early_stop=False)[0]
            err = rel(bb[b], ref)
            print(f"power {prec} L={L} M={M} n={n} B={B} plan={plan} T={T} b={b}: rel {err:.3e}")
            assert err <= TOL[prec], (T, b, err)


# ---- 2. no stale state --------------------------------------------------------

# (256, 256): k_sec4 + k_row2 (the benched single-codeword path: no zero fill,
# iters carried by the row launches); (64, 512): k_sec + k_row2
STATE_SHAPES = [(256, 256, 2048), (64, 512, 581)]


def _state_inputs(L, M, n):
    Pl = 2.0 / L * np.ones(L)
    ys = reps(L, M, n, np.tile(Pl, (2, 1)), 0.6, 700)
    rs = np.random.RandomState(9)
    b0 = np.zeros((1, L * M))
    b0[0, np.arange(L) * M + rs.randint(0, M, L)] = np.sqrt(n * Pl)
    return Pl, ys[0:1], ys[1:2], b0


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("L,M,n", STATE_SHAPES)
def test_no_stale_state(sp, prec, L, M, n):
    """A decode leaves nothing behind that a later one reads: after y1 with
    T = 6 (and after a beta0 start), y2 decoded with T = 1 and with T = 5 (odd:
    the ping-pong starts on the other side) equals, bit for bit, the same
    decode on a fresh operator."""
    Pl, y1, y2, b0 = _state_inputs(L, M, n)
    order = sp.make_ordering(L, M, n)
    if (L, M) == (256, 256):
        p = sp.SparcOperator(L, M, n, order, precision=prec).plan(1)
        assert p["section_kernel"] in ("k_sec4", "k_sec43") and p["row_kernel"] in ("k_row2", "k_row2_16"), p
    want = {}
    for T in (1, 5):
        fresh = sp.SparcOperator(L, M, n, order, precision=prec)
        fresh.reserve(1, 6)
        want[T] = decode(fresh, y2, Pl, T)
    for first in ("plain", "beta0"):
        op = sp.SparcOperator(L, M, n, order, precision=prec)
        op.reserve(1, 6)
        for T in (1, 5):
            decode(op, y1, Pl, 6, beta0=b0 if first == "beta0" else None)
            got = decode(op, y2, Pl, T)
            assert np.array_equal(got[1], want[T][1]), (first, T, got[1], want[T][1])
            assert np.array_equal(got[0], want[T][0]), (first, T)
        # and the beta0 start itself is not disturbed by what ran before it
        if first == "beta0":
            fresh = sp.SparcOperator(L, M, n, order, precision=prec)
            fresh.reserve(1, 6)
            w0 = decode(fresh, y1, Pl, 5, beta0=b0)
            g0 = decode(op, y1, Pl, 5, beta0=b0)
            assert np.array_equal(g0[0], w0[0]) and np.array_equal(g0[1], w0[1])


# ---- 3. iters and the final buffer -------------------------------------------

@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("L,M,n", STATE_SHAPES)
def test_iters_equal_T_without_stop(sp, prec, L, M, n):
    """Early stop off: iters == T for odd and even T, and the estimate fetched
    is the last iteration's whichever buffer it was written to (against the
    oracle after T iterations)."""
    Pl, y1, _, _ = _state_inputs(L, M, n)
    Ab, Az = oracle_ops(L, M, n)
    op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=prec)
    op.reserve(1, 6)
    for T in (1, 2, 5, 6):
        beta, it = decode(op, y1, Pl, T)
        assert np.array_equal(it, [T]), (T, it)
        ref = orc._amp_core(y1.reshape(-1, 1), Pl, L, M, T, Ab, Az, None, early_stop=False)[0]
        err = rel(beta[0], ref)
        print(f"final buffer {prec} L={L} M={M} T={T}: rel {err:.3e}")
        assert err <= TOL[prec], (T, err)


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("L,M,B", [(64, 64, 5), (64, 64, 1), (256, 256, 1)])
def test_early_stop_graph_equals_eager(sp, prec, L, M, B):
    """Early stop on at T = 40 (the shape and seeds of
    test_batch_matches_single_and_deterministic's (64, 64) case, and one
    codeword on the k_row2 paths): beta and iters of the captured graph equal
    those of the eager launches (plan EAGER) bit for bit, and repeat run to run."""
    P, T = 2.0, 40
    n = int(L * np.log2(M))
    Pl = P / L * np.ones(L)
    ys = reps(L, M, n, np.tile(Pl, (B, 1)), 0.6, 50)
    order = sp.make_ordering(L, M, n)
    g = sp.SparcOperator(L, M, n, order, precision=prec)
    e = sp.SparcOperator(L, M, n, order, precision=prec, plan=("EAGER",))
    bg, ig = g.amp_batch(ys, Pl, T)
    be, ie = e.amp_batch(ys, Pl, T)
    bg2, ig2 = g.amp_batch(ys, Pl, T)
    assert np.all((ig >= 0) & (ig <= T)), ig
    assert np.array_equal(ig, ie) and np.array_equal(bg, be), (ig, ie)
    assert np.array_equal(ig, ig2) and np.array_equal(bg, bg2)


# ---- 4. decisions through the pinned ring ---------------------------------------

@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("B", [1, 3])
def test_decisions_through_pinned_ring(sp, prec, B):
    """sa_decide_async's kernel writes the (B, L) indices into the pinned slot
    itself.  Three decodes of different y, slots 0 / 1 alternating, each
    collected one step behind (bench.py's protocol): every collected array is
    the argmax of that decode's fetched beta, and sa_decide agrees."""
    L, M, n, T = 64, 512, 576, 4
    Pl = 2.0 / L * np.ones(L)
    ys = reps(L, M, n, np.tile(Pl, (3 * B, 1)), 0.6, 400).reshape(3, B, n)
    op = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=prec)
    op.reserve(B, T)
    want, got = [], []
    for k in range(3):
        op.stage(ys[k], Pl)
        op.run(B, T, early_stop=False)
        op.decide_async(B, k % 2)
        if k > 0:
            got.append(op.decide_collect(B, (k - 1) % 2))
        beta, _ = op.fetch(B)
        want.append(beta.reshape(B, L, M).argmax(2).astype(np.int32))
        assert np.array_equal(op.decide(B), want[k]), k
    got.append(op.decide_collect(B, 2 % 2))
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])
    for k in range(3):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
