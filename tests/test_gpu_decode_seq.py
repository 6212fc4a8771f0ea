"""What a decode computes, whichever way its launch sequence is issued
(csrc/sa_seq.h): through the captured graph, eagerly (plan EAGER) and, where
the last section launch decides, without the fused tail (NO_FUSED_TAIL), for
T = 1, 2, 3 with the early stop on and off, from beta0 and from zero, at the
smallest shape of each one-codeword kernel family and of the batched kernel.
The estimate, iters, the decisions and z_T (sa_fetch_z runs a deferred row
step) are bit-identical across the three; the estimate is held to the oracle
by the comparison and tolerance of tests/test_gpu_sec_instances.py; and a
decode issued straight behind another one of the same context, before anything
of the first is fetched, gives what a fresh context gives (the lane's tail
state, sa_host.h: tail_begin / tail_issued / tail_beta_rewritten).  Python API
only: nothing here knows how the sequence is built."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import sec_cases as sc
import secb_cases as sbc
from oracle import amp_oracle as orc
from test_gpu_parity import TOL
from test_gpu_sec_instances import _held

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "prec L M n B plan")

_SECB = {prec: min((c for c in sbc.CASES if c.prec == prec), key=lambda c: (c.L * c.M * c.n, len(c.plan)))
         for prec in ("fp32", "fp64")}
CASES = [Case(prec, L, M, n, 1, plan) for prec in ("fp32", "fp64")
         for L, M, n, plan in ((257, 256, 509, ()), (257, 256, 509, ("SEC3",)), (257, 256, 509, ("SEC4Q",)),
                               (257, 128, 253, ()), (9, 64, 125, ()), (9, 48, 125, ()))] + \
        [Case(prec, c.L, c.M, c.n, 4, c.plan) for prec, c in _SECB.items()]
COMBOS = [(T, stop, b0) for T in (1, 2, 3) for stop in (True, False) for b0 in (False, True)]


def case_id(c):
    return f"{c.prec}-L{c.L}-M{c.M}-n{c.n}-B{c.B}" + "".join("-" + p.lower() for p in c.plan)


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


@functools.lru_cache(maxsize=None)
def _oracle_after(L, M, n, i, k, b0):
    """The oracle's estimate of codeword i after k updates from beta0 (b0) or zero, the early stop off."""
    if not b0:
        return sc.estimate_after(L, M, n, i, k)
    Ab, Az, _ = sc.fast_transforms(L, M, n)
    y = sc.inputs(L, M, n, i + 1)[i].reshape(-1, 1)
    b = orc._amp_core(y, sc.flat_power(L), L, M, k, Ab, Az, sc.start_beta0(L, M, i + 1)[i], early_stop=False)[0].reshape(-1)
    b.setflags(write=False)
    return b


def _issue(op, ys, Pl, beta0, T, stop, b0):
    """Stage and run, fetching nothing."""
    op.stage(ys, Pl, beta0=beta0 if b0 else None)
    op.run(ys.shape[0], T, early_stop=stop, beta0=b0)


def _results(op, B):
    beta, it = op.fetch(B)
    return beta, it, op.decide(B), op.fetch_z(B)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_decode_is_its_sequence_however_issued(sp, case):
    c = case
    L, M, n, B = c.L, c.M, c.n, c.B
    ordering = sp.make_ordering(L, M, n)

    def operator(*extra):
        op = sp.SparcOperator(L, M, n, ordering, precision=c.prec, plan=c.plan + extra)
        op.reserve(B, 3)
        return op

    graph, eager = operator(), operator("EAGER")
    fused = graph.plan(B)["section_kernel"] in ("k_sec4", "k_sec43", "k_sec44")
    variants = [("EAGER", eager)] + ([("NO_FUSED_TAIL", operator("NO_FUSED_TAIL"))] if fused else [])
    Pl, ys, beta0 = sc.flat_power(L), sc.inputs(L, M, n, B), sc.start_beta0(L, M, B)
    worst, res = {}, {}
    for combo in COMBOS:
        T, stop, b0 = combo
        _issue(graph, ys, Pl, beta0, *combo)
        res[combo] = r = _results(graph, B)
        for name, op in variants:
            _issue(op, ys, Pl, beta0, *combo)
            assert _same(_results(op, B), r), (combo, name)
        beta, it = r[0], r[1]
        assert np.all(it == T) if not stop else np.all((it >= 1) & (it <= T)), (combo, it)
        for i in range(B):
            _held(worst, "oracle", beta[i], _oracle_after(L, M, n, i, int(it[i]), b0), c, TOL[c.prec], (combo, i))
        # a fresh context, this decode alone
        op = operator()
        _issue(op, ys, Pl, beta0, *combo)
        assert _same(_results(op, B), r), (combo, "fresh")
        del op
    # straight behind another decode of the same context (another T, the other
    # beta0 setting), nothing of which is fetched: one context for all of them
    chain = operator()
    for T, stop, b0 in COMBOS:
        _issue(chain, ys, Pl, beta0, T % 3 + 1, stop, not b0)
        _issue(chain, ys, Pl, beta0, T, stop, b0)
        assert _same(_results(chain, B), res[(T, stop, b0)]), ((T, stop, b0), "behind another decode")
    print(f"{case_id(c)}: worst rel vs oracle {worst['oracle']:.3e}")
