"""k_row2 with its arguments as a preloaded head of 14 dwords and a tail
(csrc/sa_row2.hip): decodes held to the oracle at the suite's bounds along every
field that moved into the head or is now derived in the kernel:

  blockIdx.y strides (B = 1, 2, 3: y, z, tau, the beta^2 and Ab partials)
  tau + t folded on the host, tpos (T = 1: t = 0 alone; T = 3: tau_{t-1})
  G | Gb and T1 | flags packed (mode: the beta0 start's ROW_INIT, ROW_INIT0,
    ROW_AMP; pt: NO_PT; es: the early stop on)
  the row-block count from n (n = 600: 37.5 blocks of 16 rows; n = 601: odd)
  the beta^2 partials at an offset from tau (every decode with t > 0)
  itset and iters from the tail (fused tail on / NO_FUSED_TAIL, bit for bit)
  both row-block sizes (ROW16 / NO_ROW16) behind pairs, triples (SEC3) and
  quads (SEC4Q) of sections, packed tables or not (NO_PACK)
  two lanes against NO_LANES, bit for bit; both precisions; run-to-run equality

L = 257 has a missing section in the last pair, triple and quad.  Small shapes:
a case takes a second or two."""
import numpy as np
import pytest

import sec_cases as sc
from test_gpu_parity import TOL, argmax_agree, rel

pytestmark = pytest.mark.gpu

L = 257
SHAPES = [(256, 600), (512, 601)]
PRECS = ["fp32", "fp64"]
CASES = [(M, n, prec) for (M, n) in SHAPES for prec in PRECS]
IDS = [f"M{M}-n{n}-{prec}" for M, n, prec in CASES]


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_ORDER = {}


def make(sp, M, n, prec, plan=()):
    if (M, n) not in _ORDER:
        _ORDER[(M, n)] = sp.make_ordering(L, M, n)
    return sp.SparcOperator(L, M, n, _ORDER[(M, n)], precision=prec, plan=tuple(plan))


def held(b, ref, M, tol, what):
    e = rel(b, ref)
    print(f"{what}: rel {e:.3e} (bound {tol:.0e})")
    assert e <= tol, (what, e)
    assert argmax_agree(b, ref, L, M), what


def multiwave_row2(op, B):
    p = op.plan(B)
    return p["section_kernel"] in ("k_sec4", "k_sec43", "k_sec44") and p["row_kernel"].startswith("k_row2")


@pytest.mark.parametrize("M,n,prec", CASES, ids=IDS)
def test_batches_and_iterations(sp, M, n, prec):
    """B = 1, 2, 3 and T = 1, 3 against the oracle; a second run bit for bit."""
    op = make(sp, M, n, prec)
    Pl = sc.flat_power(L)
    for B in (1, 2, 3):
        assert multiwave_row2(op, B), op.plan(B)
        ys = sc.inputs(L, M, n, B)
        for T in (1, 3):
            bb, it = op.amp_batch(ys, Pl, T, early_stop=False)
            assert np.all(it == T), it
            for i in range(B):
                held(bb[i], sc.estimate_after(L, M, n, i, T), M, TOL[prec], ("fixed", B, T, i))
            b2, it2 = op.amp_batch(ys, Pl, T, early_stop=False)
            assert np.array_equal(b2, bb) and np.array_equal(it2, it)


@pytest.mark.parametrize("M,n,prec", CASES, ids=IDS)
def test_beta0_start(sp, M, n, prec):
    """The start from an estimate: ROW_INIT on the [G][n] partials of the start's own A beta0."""
    B = 2
    op = make(sp, M, n, prec)
    ys, b0, refs = sc.inputs(L, M, n, B), sc.start_beta0(L, M, B), sc.start_reference(L, M, n, B)
    bs, its = op.amp_batch(ys, sc.flat_power(L), sc.T_START, beta0=b0, early_stop=False)
    assert np.all(its == sc.T_START), its
    for i in range(B):
        held(bs[i], refs[i], M, TOL[prec], ("beta0 start", i))


@pytest.mark.parametrize("M,n,prec", CASES, ids=IDS)
def test_early_stop(sp, M, n, prec):
    """The early stop on: the estimate against the oracle's at the stop index
    the device reports (iters = t: t updates; T: the loop ran out)."""
    B = 2
    op = make(sp, M, n, prec)
    ys = sc.inputs(L, M, n, B)
    be, ite = op.amp_batch(ys, sc.flat_power(L), sc.T_STOP)
    assert np.all((ite >= 1) & (ite <= sc.T_STOP)), ite
    for i in range(B):
        held(be[i], sc.estimate_after(L, M, n, i, int(ite[i])), M, TOL[prec], ("early stop", i, int(ite[i])))
    be2, ite2 = op.amp_batch(ys, sc.flat_power(L), sc.T_STOP)
    assert np.array_equal(be2, be) and np.array_equal(ite2, ite)


@pytest.mark.parametrize("plan", [("NO_PACK",), ("SEC3",), ("SEC4Q",), ("ROW16",), ("NO_ROW16",), ("NO_PT",),
                                  ("SEC4Q", "NO_ROW16")], ids=lambda p: "-".join(p).lower())
@pytest.mark.parametrize("M,n,prec", CASES, ids=IDS)
def test_plan_variants(sp, M, n, prec, plan):
    """Every producer of k_row2's partials and both of its row-block sizes, B = 1 and 2, T = 3."""
    op = make(sp, M, n, prec, plan)
    Pl, T = sc.flat_power(L), 3
    p1 = op.plan(1)
    assert p1["row_kernel"].startswith("k_row2"), p1
    if "NO_ROW16" in plan:
        assert p1["row_kernel"] == "k_row2", p1
    if "SEC3" in plan:
        assert p1["section_kernel"] == "k_sec43", p1
    if "SEC4Q" in plan:
        assert p1["section_kernel"] == "k_sec44", p1
    for B in (1, 2):
        ys = sc.inputs(L, M, n, B)
        bb, it = op.amp_batch(ys, Pl, T, early_stop=False)
        assert np.all(it == T), it
        for i in range(B):
            held(bb[i], sc.estimate_after(L, M, n, i, T), M, TOL[prec], (plan, B, i))


@pytest.mark.parametrize("M,n,prec", CASES, ids=IDS)
def test_fused_tail_bit_for_bit(sp, M, n, prec):
    """The fused tail (the last row launch deferred, iters from the section kernel)
    and NO_FUSED_TAIL (k_row2 writes iters = T through its tail): the same bits."""
    Pl, T = sc.flat_power(L), 3
    a, b = make(sp, M, n, prec), make(sp, M, n, prec, ("NO_FUSED_TAIL",))
    for B in (1, 3):
        ys = sc.inputs(L, M, n, B)
        ba, ia = a.amp_batch(ys, Pl, T, early_stop=False)
        bb, ib = b.amp_batch(ys, Pl, T, early_stop=False)
        assert np.array_equal(ba, bb) and np.array_equal(ia, ib) and np.all(ib == T)
        assert np.array_equal(a.decide(B), b.decide(B))


def pipelined(op, ys, Pl, T):
    """bench.py's protocol: stage, run, decide_async(k % 2), collect step k - 1."""
    got = []
    for k, y in enumerate(ys):
        op.stage(y, Pl, None)
        op.run(1, T, early_stop=False)
        op.decide_async(1, k % 2)
        if k > 0:
            got.append(op.decide_collect(1, (k - 1) % 2))
    got.append(op.decide_collect(1, (len(ys) - 1) % 2))
    return got


@pytest.mark.parametrize("M,n,prec", CASES, ids=IDS)
def test_lanes_bit_for_bit(sp, M, n, prec):
    """Four words through two lanes and through one (NO_LANES): the same
    decisions, and the last decode's estimate, residual and iters bit for bit."""
    Pl, T = sc.flat_power(L), 3
    ys = [sc.inputs(L, M, n, 3)[i % 3].reshape(1, -1) for i in range(4)]
    two, one = make(sp, M, n, prec), make(sp, M, n, prec, ("NO_LANES",))
    for op in (two, one):
        op.reserve(1, T)
    g2, g1 = pipelined(two, ys, Pl, T), pipelined(one, ys, Pl, T)
    for k in range(len(ys)):
        assert np.array_equal(g2[k], g1[k]), k
        assert np.array_equal(g2[k][0], sc.estimate_after(L, M, n, k % 3, T).reshape(L, M).argmax(1)), k
    (b2, i2), (b1, i1) = two.fetch(1), one.fetch(1)
    assert np.array_equal(b2, b1) and np.array_equal(i2, i1)
    assert np.array_equal(two.fetch_z(1), one.fetch_z(1))
