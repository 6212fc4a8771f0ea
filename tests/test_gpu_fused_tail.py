"""Fused tail of a one-codeword decode with the early stop off: the last
section launch of k_sec4 / k_sec43 / k_sec44 writes the section decisions and
iters, k_decide is never launched, and the last k_row2 step (z_T, read by
sa_fetch_z alone) runs only on demand.  Plan option NO_FUSED_TAIL keeps the
former sequence; no arithmetic differs, so every case compares the two plans
on the same inputs bit for bit (np.array_equal): decisions from decide_async /
decide_collect and from decide, beta and iters from fetch, z from fetch_z.
Where beta is finite the decisions also equal np.argmax of each fetched
section (first index on ties).

Shapes.  The multi-wave section kernels run a single codeword only from
ceil(L / 2) * 2 >= the CU count, so L = 5 (a missing section in the last pair,
one in the last triple, three in the last quad) takes k_sec and with it
k_decide under either plan; L = 257 = 5 + 12 * 21 leaves the same sections
missing and does run the pair / triple (SEC3) / quad (SEC4Q) kernels, so both
are here.  M = 256, 512 (one and two registers per lane and wave); n = 600 and
601 in binary32 (a whole number of 16-byte z pieces, then not), 601 in
binary64; T = 1 (the fused launch is also the bzero launch), 2, 3 (both
parities of the ping-pong)."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

MULTI = ("k_sec4", "k_sec43", "k_sec44")
OFF = ("NO_FUSED_TAIL",)


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_ORDER, _Y = {}, {}


def ordering(sp, L, M, n):
    if (L, M, n) not in _ORDER:
        _ORDER[(L, M, n)] = sp.make_ordering(L, M, n)
    return _ORDER[(L, M, n)]


def power(L, P=2.0):
    return P / L * np.ones(L)


def word(n, seed):
    """A received word (1, n) of the channel's scale (P = 2, sigma = 0.6), built once."""
    if (n, seed) not in _Y:
        _Y[(n, seed)] = np.sqrt(2.36) * np.random.RandomState(seed).randn(1, n)
    return _Y[(n, seed)]


def make(sp, shape, prec, plan=()):
    L, M, n = shape
    op = sp.SparcOperator(L, M, n, ordering(sp, L, M, n), precision=prec, plan=tuple(plan) or None)
    op.reserve(1, 4)
    return op


def results(op, T, es=False, beta0=False):
    """Everything a caller can read after one run of the staged word."""
    op.run(1, T, early_stop=es, beta0=beta0)
    op.decide_async(1, 0)
    out = dict(dec_async=op.decide_collect(1, 0), dec=op.decide(1))
    out["beta"], out["iters"] = op.fetch(1)
    out["z"] = op.fetch_z(1)
    out["z_again"] = op.fetch_z(1)  # the deferred row step has run: nothing is launched
    return out


def same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert np.array_equal(a["z"], a["z_again"], equal_nan=True), what
    assert np.array_equal(a["dec"], a["dec_async"]), what


def check_argmax(r, L, M, what=""):
    beta = r["beta"].reshape(L, M)
    if np.isfinite(beta).all():
        assert np.array_equal(r["dec"].reshape(-1), np.argmax(beta, axis=1)), what


SHAPES = [((257, 256, 600), "fp32"), ((257, 256, 601), "fp32"), ((257, 512, 600), "fp32"), ((257, 512, 601), "fp64"),
          ((5, 256, 601), "fp32")]


@pytest.mark.parametrize("extra", [(), ("SEC3",), ("SEC4Q",)], ids=["pairs", "triples", "quads"])
@pytest.mark.parametrize("shape,prec", SHAPES)
def test_plans_bit_identical(sp, shape, prec, extra):
    """T = 1, 2, 3 on one operator per plan; then a beta0 start (no bzero
    launch, the estimate ends on either side), the early stop on (the fallback:
    k_decide, iters from k_row2 or the stop), and y = 0 (every value of a
    section equal or NaN: a tie)."""
    L, M, n = shape
    Pl, y = power(L), word(n, 11)
    on, off = make(sp, shape, prec, extra), make(sp, shape, prec, extra + OFF)
    plan = on.plan(1)
    assert plan == off.plan(1)
    if L >= 256:
        assert plan["section_kernel"] in MULTI and plan["row_kernel"].startswith("k_row2"), plan
        assert plan["section_kernel"] == {(): "k_sec4", ("SEC3",): "k_sec43", ("SEC4Q",): "k_sec44"}[extra]
    for op in (on, off):
        op.stage(y, Pl)
    for T in (1, 2, 3):
        a, b = results(on, T), results(off, T)
        same(a, b, ("T", T))
        check_argmax(a, L, M, ("T", T))
        assert a["iters"][0] == T
    beta0 = 0.05 * np.abs(np.random.RandomState(5).randn(1, L * M))
    for T in (2, 3):
        for op in (on, off):
            op.stage(y, Pl, beta0)
        a, b = results(on, T, beta0=True), results(off, T, beta0=True)
        same(a, b, ("beta0", T))
        check_argmax(a, L, M, ("beta0", T))
    for op in (on, off):
        op.stage(y, Pl)
    a, b = results(on, 3, es=True), results(off, 3, es=True)
    same(a, b, "early stop")
    check_argmax(a, L, M, "early stop")
    for op in (on, off):
        op.stage(np.zeros((1, n)), Pl)
    a, b = results(on, 2), results(off, 2)
    same(a, b, "tie")
    check_argmax(a, L, M, "tie")


def reference(sp, shape, prec, y, T):
    """One decode on a fresh single-lane operator with the former sequence."""
    op = make(sp, shape, prec, ("NO_LANES",) + OFF)
    op.stage(y, power(shape[0]))
    return results(op, T)


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_lanes_one_step_behind(sp, prec):
    """bench.py's protocol for eight steps, y staged at step 0 and again at
    step 3 (the lanes copy it over): every collected decision is that of the y
    its step decoded, with and without lanes, with and without the fused tail;
    fetch and fetch_z afterwards are the last step's."""
    shape, T = (257, 256, 601), 3
    L, M, n = shape
    Pl, ys = power(L), [word(n, 21), word(n, 22)]
    refs = [reference(sp, shape, prec, y, T) for y in ys]
    assert not np.array_equal(refs[0]["dec"], refs[1]["dec"])
    for plan in ((), ("NO_LANES",), OFF, ("NO_LANES",) + OFF):
        op = make(sp, shape, prec, plan)
        got, want = [], []
        for k in range(8):
            if k in (0, 3):
                op.stage(ys[0 if k == 0 else 1], Pl)
            want.append(refs[0 if k < 3 else 1])
            op.run(1, T, early_stop=False)
            op.decide_async(1, k % 2)
            if k > 0:
                got.append(op.decide_collect(1, (k - 1) % 2))
        got.append(op.decide_collect(1, 7 % 2))
        for k in range(8):
            assert np.array_equal(got[k], want[k]["dec"]), (plan, k)
        beta, it = op.fetch(1)
        assert np.array_equal(beta, refs[1]["beta"]) and np.array_equal(it, refs[1]["iters"]), plan
        assert np.array_equal(op.fetch_z(1), refs[1]["z"]), plan
        assert np.array_equal(op.decide(1), refs[1]["dec"]), plan


@pytest.mark.parametrize("plan", [(), ("NO_LANES",), OFF], ids=["lanes", "one_lane", "unfused"])
def test_three_runs_before_any_collect(sp, plan):
    """Three steps (a new y each) queued into three slots with no collect in
    between, then the collects: a lane is reused while a slot still points at
    its decisions, which move into the ring first.  Every slot yields its own
    step's decisions."""
    shape, prec, T = (257, 256, 600), "fp32", 2
    L, M, n = shape
    Pl, ys = power(L), [word(n, 31 + i) for i in range(3)]
    refs = [reference(sp, shape, prec, y, T) for y in ys]
    op = make(sp, shape, prec, plan)
    for k, y in enumerate(ys):
        op.stage(y, Pl)
        op.run(1, T, early_stop=False)
        op.decide_async(1, k)
    for k in (2, 0, 1):
        assert np.array_equal(op.decide_collect(1, k), refs[k]["dec"]), k
    assert np.array_equal(op.fetch_z(1), refs[2]["z"])


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_run_straight_after_a_pending_row_step(sp, prec):
    """A run issued while the previous run's row step is still deferred drops
    it (z starts from y again); a y staged over a deferred row step does not
    change the z of the decode that ran before it."""
    shape, T = (257, 512, 601), 3
    L, M, n = shape
    Pl, ya, yb = power(L), word(n, 41), word(n, 42)
    ra, rb = reference(sp, shape, prec, ya, T), reference(sp, shape, prec, yb, T)
    op = make(sp, shape, prec, ("NO_LANES",))
    op.stage(ya, Pl)
    op.run(1, T, early_stop=False)
    op.run(1, T, early_stop=False)  # the first run's row step never runs
    op.wait()
    assert np.array_equal(op.fetch_z(1), ra["z"]) and np.array_equal(op.decide(1), ra["dec"])
    op.run(1, T, early_stop=False)
    op.stage(yb, Pl)  # the deferred row step reads ya: it runs in front of the upload
    assert np.array_equal(op.fetch_z(1), ra["z"])
    beta, it = op.fetch(1)
    assert np.array_equal(beta, ra["beta"]) and np.array_equal(it, ra["iters"])
    same(results(op, T), rb, "restaged")


def test_c2_once(sp):
    """The bench shape (L = M = 512, n = 4608, binary32) at T = 4."""
    g = golden("c2.npz")
    L, M, n = int(g["L"]), int(g["M"]), int(g["n"])
    y = np.asarray(g["y"], dtype=np.float64).reshape(1, -1)
    Pl = float(g["P"]) / L * np.ones(L)
    on, off = make(sp, (L, M, n), "fp32"), make(sp, (L, M, n), "fp32", OFF)
    assert on.plan(1)["section_kernel"] == "k_sec4"
    for op in (on, off):
        op.stage(y, Pl)
    a, b = results(on, 4), results(off, 4)
    same(a, b, "c2")
    check_argmax(a, L, M, "c2")
