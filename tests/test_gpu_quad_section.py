"""k_sec44: four sections x four waves per workgroup on the pair table (plan
option SEC4Q; sa_sec.hip).  Quads regroup a row's partial sum as pair sums
first, (+-v0 +- v1) + (+-v2 +- v3), so they are compared with the oracle at
TOL and with the pair kernel within 2 TOL, never bit for bit; a laned and a
lone decode of the same plan are bit-identical.  Shapes: the smallest with a
missing pair / a missing section in the last workgroup, n past one 5 x 1024
row pass, n * sizeof(real) no multiple of the 16-byte LDS-DMA piece, and c2
itself (G = 128: k_row2's constant-stride path at 4 / 8 loads per thread)."""
import numpy as np
import pytest

from conftest import golden
from oracle import amp_oracle as orc
from test_gpu_parity import TOL, argmax_agree, rel

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "fp64"]
PARTIALS = {"k_sec4": 2, "k_sec43": 3, "k_sec44": 4}  # sections per Ab partial


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


_CASE = {}


def case(L, M, n):
    """Oracle operator, ordering, Pl, one y and a cache of oracle decodes by t
    (computed once per shape, shared by both precisions and every test)."""
    key = (L, M, n)
    if key not in _CASE:
        oAb, oAz, oord = orc.sparc_transforms(L, M, n)
        Pl = 2.0 / L * np.ones(L)
        y = orc.rep_inputs(L, M, n, Pl, 0.9, oAb, 300)[1].reshape(-1)
        _CASE[key] = dict(oAb=oAb, oAz=oAz, oord=oord, Pl=Pl, y=y, ref={})
    return _CASE[key]


def oracle_at(c, L, M, t):
    if t not in c["ref"]:
        c["ref"][t] = orc.amp_test(c["y"], 0, c["Pl"], L, M, t, c["oAb"], c["oAz"])[0]
    return c["ref"][t]


def c2_case():
    """c2 (L = M = 512, n = 4608) with the golden y; oracle decodes cached by t."""
    if "c2" not in _CASE:
        g = golden("c2.npz")
        L, M, n = int(g["L"]), int(g["M"]), int(g["n"])
        oAb, oAz, oord = orc.sparc_transforms(L, M, n)
        _CASE["c2"] = dict(L=L, M=M, n=n, oAb=oAb, oAz=oAz, oord=oord, Pl=float(g["P"]) / L * np.ones(L),
                           y=np.asarray(g["y"], dtype=np.float64).reshape(-1), ref={})
    return _CASE["c2"]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("L,M,n", [(258, 512, 2580), (257, 256, 2284), (300, 512, 6000), (258, 256, 2581)])
def test_quads_vs_oracle_and_pairs(sp, prec, L, M, n):
    """Forced SEC4Q against the oracle per iteration (t = 1, 2, 5) and against
    forced pairs within 2 TOL; the plan it reports; two 30-iteration
    early-stop decodes bitwise reproducible."""
    c = case(L, M, n)
    Pl, y = c["Pl"], c["y"].reshape(1, -1)
    q = sp.SparcOperator(L, M, n, c["oord"], precision=prec, plan="SEC4Q")
    p = sp.SparcOperator(L, M, n, c["oord"], precision=prec, plan=("NO_SEC3", "NO_SEC4Q"))
    assert q.plan(1)["section_kernel"] == "k_sec44"
    assert q.plan(1)["partials"] == (L + 3) // 4
    assert p.plan(1)["section_kernel"] == "k_sec4"
    for t in (1, 2, 5):
        ref = oracle_at(c, L, M, t)
        b4, _ = q.amp_batch(y, Pl, t, early_stop=False)
        b2, _ = p.amp_batch(y, Pl, t, early_stop=False)
        e4, e2 = rel(b4[0], ref), rel(b4[0], b2[0])
        print(f"quads {prec} L={L} M={M} n={n} t={t}: vs oracle {e4:.3e}, vs pairs {e2:.3e}")
        assert e4 <= TOL[prec], t
        assert e2 <= 2 * TOL[prec], t
    b, i = q.amp_batch(y, Pl, 30)
    bb, ib = q.amp_batch(y, Pl, 30)
    assert np.array_equal(b, bb) and np.array_equal(i, ib)  # bitwise reproducible
    if 30 not in c["ref"]:
        c["ref"][30] = orc.amp(c["y"], 0, Pl, L, M, 30, c["oAb"], c["oAz"])
    assert argmax_agree(b[0], c["ref"][30], L, M)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", ["c2", (258, 512, 2580)])
def test_quads_row_block_widths(sp, prec, shape):
    """The same decode with 16-row and with 32-row k_row2 blocks under SEC4Q,
    each against the oracle: at c2 (G = 128) k_row2's constant-stride path at
    U = 4 (16-row) and U = 8 (32-row, binary32), elsewhere its general loop."""
    if shape == "c2":
        c = c2_case()
        L, M, n = c["L"], c["M"], c["n"]
    else:
        L, M, n = shape
        c = case(L, M, n)
    Pl, y = c["Pl"], c["y"].reshape(1, -1)
    for rows, kern in (("ROW16", "k_row2_16"), ("NO_ROW16", "k_row2")):
        op = sp.SparcOperator(L, M, n, c["oord"], precision=prec, plan=("SEC4Q", rows))
        plan = op.plan(1)
        assert plan["section_kernel"] == "k_sec44" and plan["row_kernel"] == kern, plan
        if shape == "c2":
            assert plan["partials"] == 128
        for t in (1, 5):
            b, _ = op.amp_batch(y, Pl, t, early_stop=False)
            err = rel(b[0], oracle_at(c, L, M, t))
            print(f"quads {rows} {prec} L={L} n={n} t={t}: vs oracle {err:.3e}")
            assert err <= TOL[prec], (rows, t)


@pytest.mark.parametrize("prec", PRECS)
def test_quads_lanes_bit_identical(sp, prec):
    """(256, 256, 2048) with SEC4Q: a three-step one-behind ring (run,
    decide_async, decide_collect) on the decode lanes against the same ring
    on a NO_LANES operator: decisions, beta and iters equal bit for bit."""
    L, M, n, T = 256, 256, 2048, 5
    oAb, _, oord = orc.sparc_transforms(L, M, n)
    Pl = 2.0 / L * np.ones(L)
    ys = [orc.rep_inputs(L, M, n, Pl, 0.9, oAb, 500 + i)[1].reshape(1, -1) for i in range(3)]
    out = {}
    for name, plan in (("lanes", ("SEC4Q",)), ("one", ("SEC4Q", "NO_LANES"))):
        op = sp.SparcOperator(L, M, n, oord, precision=prec, plan=plan)
        assert op.plan(1)["section_kernel"] == "k_sec44"
        op.reserve(1, 6)
        dec = []
        for k, y in enumerate(ys):
            op.stage(y, Pl)
            op.run(1, T, early_stop=True)
            op.decide_async(1, k % 2)
            if k > 0:
                dec.append(op.decide_collect(1, (k - 1) % 2))
        dec.append(op.decide_collect(1, (len(ys) - 1) % 2))
        beta, iters = op.fetch(1)
        out[name] = (dec, beta, iters)
    assert not np.array_equal(out["one"][0][0], out["one"][0][1])  # the steps differ
    for k in range(3):
        assert np.array_equal(out["lanes"][0][k], out["one"][0][k]), k
    assert np.array_equal(out["lanes"][1], out["one"][1])
    assert np.array_equal(out["lanes"][2], out["one"][2])


@pytest.mark.parametrize("prec", PRECS)
def test_quads_c2_vs_oracle(sp, prec):
    """c2 itself with SEC4Q, T = 5, against the oracle at TOL."""
    c = c2_case()
    L, M, n = c["L"], c["M"], c["n"]
    op = sp.SparcOperator(L, M, n, c["oord"], precision=prec, plan="SEC4Q")
    assert op.plan(1)["section_kernel"] == "k_sec44" and op.plan(1)["partials"] == 128
    b, _ = op.amp_batch(c["y"].reshape(1, -1), c["Pl"], 5, early_stop=False)
    err = rel(b[0], oracle_at(c, L, M, 5))
    print(f"quads c2 {prec} T=5: vs oracle {err:.3e}")
    assert err <= TOL[prec]


def test_chooser(sp):
    """What the built-in rule may pick: (256, 256, 2048) keeps pairs or
    triples; L = 768 follows test_c4_single_uses_triples' rule; whatever c2
    reports has the partial count of its kernel."""
    op = sp.SparcOperator(256, 256, 2048, sp.make_ordering(256, 256, 2048))
    assert op.plan(1)["section_kernel"] in ("k_sec4", "k_sec43"), op.plan(1)
    L, M = 768, 512
    n = int(L * np.log2(M) / (5 / 6))
    plan = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n)).plan(1)
    want = "k_sec43" if (L + 1) // 2 > plan["cus"] >= (L + 2) // 3 else "k_sec4"
    assert plan["section_kernel"] == want, plan
    assert plan["partials"] == (256 if want == "k_sec43" else 384)
    for prec in PRECS:
        L, M, n = 512, 512, 4608
        plan = sp.SparcOperator(L, M, n, sp.make_ordering(L, M, n), precision=prec).plan(1)
        assert plan["section_kernel"] in PARTIALS, plan
        per = PARTIALS[plan["section_kernel"]]
        assert plan["partials"] == (L + per - 1) // per, plan
