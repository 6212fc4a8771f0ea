"""The packed tables of the pair and quad section kernels (k_sec4, k_sec44;
csrc/sa_sec.hip: secq_body's PKI / PKF bodies): 13-bit bucket records and three
pair-table rows per 64-bit word unpack to the values inv and fwd2 hold, so a
decode on them equals the decode of a NO_PACK operator bit for bit (beta, z,
iters, the decisions of the fused tail and of k_decide) and stays within the
section kernels' bound of the oracle, iteration by iteration.

Shapes of tests/test_packed_tables_host.py at L = 257: 129 pairs, the last
with one section; with SEC4Q 65 quads, the last with one section."""
import numpy as np
import pytest

import sec_cases as sc
from test_gpu_decode_lanes import pipelined
from test_gpu_parity import TOL, argmax_agree, rel

pytestmark = pytest.mark.gpu

L = 257
SHAPES = [(512, 1021), (512, 4608), (512, 4609), (256, 8190), (256, 509)]
PRECS = ["fp32", "fp64"]
T = 3
KERNEL = {(): "k_sec4", ("SEC4Q",): "k_sec44"}


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_ORDER = {}


def make(sp, M, n, prec, plan=()):
    if (M, n) not in _ORDER:
        _ORDER[(M, n)] = sp.make_ordering(L, M, n)
    return sp.SparcOperator(L, M, n, _ORDER[(M, n)], precision=prec, plan=tuple(plan))


def packed_bytes(M, n, prec, quads):
    """Device bytes of the packed tables (csrc/sa_shape.h: pack_rd, pack_fwd_words)."""
    w = 1 << (max(M + 1, n + 1) - 1).bit_length()
    kh = 8 if quads and prec == "fp64" else 16
    rd, blocks = ((M // 256) * kh * 13 + 31) // 32, (w // M + kh - 1) // kh
    invp = L * 4 * blocks * 64 * rd * 4
    fwd2p = 0 if quads else (L + 1) // 2 * 3 * ((n + 4607) // 4608) * 512 * 8
    return invp + fwd2p


def decode(op, ys, Pl, T, es, beta0=None):
    """One decode of ys (B, n): beta, iters, z and the decisions (the fused
    tail's with the early stop off, k_decide's with it on)."""
    B = ys.shape[0]
    op.reserve(B, 8)
    op.stage(ys, Pl, beta0)
    op.run(B, T, early_stop=es, beta0=beta0 is not None)
    op.wait()
    beta, it = op.fetch(B)
    return dict(beta=beta, iters=it, dec=op.decide(B), z=op.fetch_z(B))


def same(a, b, what):
    for k in ("beta", "iters", "dec", "z"):
        assert np.array_equal(a[k], b[k]), (what, k)


def held(b, ref, M, prec, what):
    e = rel(b, ref)
    print(f"{what}: rel {e:.3e} (bound {TOL[prec]:.0e})")
    assert e <= TOL[prec], (what, e)
    assert argmax_agree(b, ref, L, M), what


@pytest.mark.parametrize("plan", [(), ("SEC4Q",)], ids=["pairs", "quads"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("M,n", SHAPES)
def test_packed_equals_no_pack_and_holds_the_oracle(sp, M, n, prec, plan):
    op, op0 = make(sp, M, n, prec, plan), make(sp, M, n, prec, plan + ("NO_PACK",))
    if op.plan(1)["cus"] != sc.N_CUS:
        pytest.skip(f"the kernel choice is written for {sc.N_CUS} CUs")
    for o in (op, op0):
        assert o.plan(1)["section_kernel"] == KERNEL[plan], o.plan(1)
    # the packed tables exist on one operator and not on the other
    assert op.info()["device_bytes"] - op0.info()["device_bytes"] == packed_bytes(M, n, prec, bool(plan))
    Pl, ys = sc.flat_power(L), sc.inputs(L, M, n, 1)
    for es in (False, True):
        for t in range(1, T + 1):
            a, a0 = decode(op, ys, Pl, t, es), decode(op0, ys, Pl, t, es)
            same(a, a0, (es, t))
            it = int(a["iters"][0])
            assert 1 <= it <= t and (es or it == t), (es, t, it)
            held(a["beta"][0], sc.estimate_after(L, M, n, 0, it), M, prec, f"es={es} T={t} iters={it}")
            assert np.array_equal(a["dec"][0], a["beta"][0].reshape(L, M).argmax(1))


@pytest.mark.parametrize("plan", [(), ("SEC4Q",)], ids=["pairs", "quads"])
@pytest.mark.parametrize("prec", PRECS)
def test_beta0_start(sp, prec, plan):
    """A decode from beta0: the first pair launch reads an estimate (no bzero)."""
    M, n = 512, 1021
    Pl, ys = sc.flat_power(L), sc.inputs(L, M, n, 1)
    b0 = sc.start_beta0(L, M, 1)
    op, op0 = make(sp, M, n, prec, plan), make(sp, M, n, prec, plan + ("NO_PACK",))
    if op.plan(1)["cus"] != sc.N_CUS:
        pytest.skip(f"the kernel choice is written for {sc.N_CUS} CUs")
    a = decode(op, ys, Pl, sc.T_START, False, b0)
    same(a, decode(op0, ys, Pl, sc.T_START, False, b0), "beta0")
    held(a["beta"][0], sc.start_reference(L, M, n, 1)[0], M, prec, "beta0 start")


@pytest.mark.parametrize("plan", [(), ("SEC4Q",)], ids=["pairs", "quads"])
@pytest.mark.parametrize("M,n,B", [(256, 509, 2), (512, 1021, 3)])
@pytest.mark.parametrize("prec", PRECS)
def test_batches_through_grid_y(sp, prec, M, n, B, plan):
    Pl, ys = sc.flat_power(L), sc.inputs(L, M, n, B)
    op, op0 = make(sp, M, n, prec, plan), make(sp, M, n, prec, plan + ("NO_PACK",))
    if op.plan(B)["cus"] != sc.N_CUS:
        pytest.skip(f"the kernel choice is written for {sc.N_CUS} CUs")
    assert op.plan(B)["section_kernel"] == KERNEL[plan]
    for es in (False, True):
        a = decode(op, ys, Pl, T, es)
        same(a, decode(op0, ys, Pl, T, es), es)
        for i in range(B):
            held(a["beta"][i], sc.estimate_after(L, M, n, i, int(a["iters"][i])), M, prec, f"B={B} codeword {i} es={es}")


@pytest.mark.parametrize("prec", PRECS)
def test_two_lanes_one_step_behind(sp, prec):
    """Four different y through the two decode lanes, each step's decisions
    collected one step later: the packed operator against a NO_PACK operator on
    one lane, fed the same stream, and against each input's own decode."""
    M, n = 512, 4608
    Pl, ys = sc.flat_power(L), sc.inputs(L, M, n, 4)
    steps = [(ys[i:i + 1], Pl, T, False, None) for i in range(4)]
    op, op0 = make(sp, M, n, prec), make(sp, M, n, prec, ("NO_PACK", "NO_LANES"))
    if op.plan(1)["cus"] != sc.N_CUS:
        pytest.skip(f"the kernel choice is written for {sc.N_CUS} CUs")
    op.reserve(1, 8)
    op0.reserve(1, 8)
    got, got0 = pipelined(op, steps), pipelined(op0, steps)
    for k in range(4):
        assert np.array_equal(got[k], got0[k]), k
    assert not np.array_equal(got[0], got[1])
    beta, it = op.fetch(1)
    beta0, it0 = op0.fetch(1)
    assert np.array_equal(beta, beta0) and np.array_equal(it, it0)
    assert np.array_equal(op.fetch_z(1), op0.fetch_z(1))
    ref = decode(make(sp, M, n, prec, ("NO_PACK", "NO_LANES")), ys[3:4], Pl, T, False)
    assert np.array_equal(beta, ref["beta"]) and np.array_equal(got[3], ref["dec"])
