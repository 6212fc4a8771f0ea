"""Every selectable k_secb instance (csrc/sa_secb.hip) at a small shape
against the oracle: one test id per case of tests/secb_cases.py.  Each case
proves through the plan report which instance it ran, so a bad instance costs
its own ids and no others.  The shapes (L = W + 3, B = 7 or 5) give two
section groups with 3 live waves in the second and a partial last chunk."""
import numpy as np
import pytest

import secb_cases as sc
from oracle import amp_oracle as orc
from test_gpu_parity import STOP32_EARLY, STOP64, TOL, argmax_agree, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


def _operator(sp, c):
    """The case's operator, after its plan report proved the instance (a
    mismatch here is a fault of the case table or the host model)."""
    op = sp.SparcOperator(c.L, c.M, c.n, sp.make_ordering(c.L, c.M, c.n), precision=c.prec, plan=c.plan)
    for B in (c.B, c.B - 1, 4):
        p = op.plan(B)
        assert p["section_kernel"] == "k_secb", p
        assert p["codewords_per_wg"] == c.CB, p
        assert op.plan_batched(B)["sections_per_wg"] == c.W
        assert (p["row_kernel"] == "k_rowc") == c.ZIL, p
    assert op.plan(1)["section_kernel"] != "k_secb"
    return op


@pytest.mark.parametrize("case", sc.CASES + sc.NOBANKS_CASES, ids=sc.case_id)
def test_instance_vs_oracle(sp, case):
    c = case
    op = _operator(sp, c)
    T, Pl = sc.T_FIXED, sc.flat_power(c.L)
    ys, refs = sc.fixed_reference(c.L, c.M, c.n, c.B)
    # (b) every codeword against the oracle
    bb, it = op.amp_batch(ys, Pl, T, early_stop=False)
    errs = [rel(bb[i], refs[i]) for i in range(c.B)]
    # (c) against the one-codeword path of the same operator
    errs1 = []
    for i in range(c.B):
        b1, _ = op.amp_batch(ys[i:i + 1], Pl, T, early_stop=False)
        errs1.append(rel(bb[i], b1[0]))
    print(f"{sc.case_id(c)}: worst rel vs oracle {max(errs):.3e}, vs one-codeword decode {max(errs1):.3e}")
    for i in range(c.B):
        assert errs[i] <= TOL[c.prec], (i, errs[i])
        assert argmax_agree(bb[i], refs[i], c.L, c.M), i
        assert errs1[i] <= 2 * TOL[c.prec], (i, errs1[i])
    assert np.all(it == T), it
    # (d) bit for bit wherever the codeword sits in the batch: no arithmetic
    # crosses codewords and every reduction has a fixed order
    b2, it2 = op.amp_batch(ys, Pl, T, early_stop=False)
    assert np.array_equal(b2, bb) and np.array_equal(it2, it)
    br, itr = op.amp_batch(ys[::-1], Pl, T, early_stop=False)
    assert np.array_equal(br[::-1], bb) and np.all(itr == T)
    bt, itt = op.amp_batch(ys[1:], Pl, T, early_stop=False)
    assert np.all(itt == T)
    if op.plan(c.B - 1)["row_kernel"] == op.plan(c.B)["row_kernel"]:
        assert np.array_equal(bt, bb[1:])
    else:
        # the row kernel is chosen by B (plan_for: k_row2 below 4 CUs' worth of
        # 64-row blocks) and each one sums z^2 in blocks of its own size, so tau
        # of B - 1 codewords may round differently; the
        # bits must still not depend on the slot at this B: every codeword
        # moved by one slot, with other chunk-mates
        assert all(rel(bt[i], bb[1 + i]) <= TOL[c.prec] for i in range(c.B - 1))
        bs, its = op.amp_batch(np.roll(ys, 1, axis=0), Pl, T, early_stop=False)
        assert np.array_equal(np.roll(bs, -1, axis=0), bb) and np.all(its == T)


@pytest.mark.parametrize("case", sc.STOP_CASES, ids=sc.case_id)
def test_early_stop_inside_a_chunk(sp, case):
    """Codewords that stop early (even i) beside ones that run on (odd i) in
    one chunk: frozen beside live chunk-mates in the mixed batch, the
    whole-workgroup return in the batches of four copies of one codeword."""
    c = case
    op = _operator(sp, c)
    T, Pl = sc.T_STOP, sc.flat_power(c.L)
    idx, ys, refs, t_ref, upd = sc.stop_reference(c.L, c.M, c.n, c.B)
    # (the row kernel, and with it the order of tau's sum, follows B: the same one at both sizes)
    assert op.plan(4)["row_kernel"] == op.plan(c.B)["row_kernel"]
    bm, itm = op.amp_batch(ys, Pl, T)
    bm2, itm2 = op.amp_batch(ys, Pl, T)
    assert np.array_equal(bm2, bm) and np.array_equal(itm2, itm)
    print(f"{sc.case_id(c)}: stop indices {itm.tolist()}, oracle {t_ref.tolist()}")
    for i in range(c.B):
        bh, ith = op.amp_batch(np.tile(ys[i], (4, 1)), Pl, T)
        assert np.all(ith == itm[i]), (i, ith, itm[i])
        assert all(np.array_equal(bh[k], bm[i]) for k in range(4)), i
    for i in range(c.B):
        t = min(int(itm[i]), T - 1)
        if c.prec == "fp64":
            assert abs(t - t_ref[i]) <= STOP64, (i, itm, t_ref)
            if int(itm[i]) == upd[i]:  # the same number of updates behind both estimates
                assert rel(bm[i], refs[i]) <= TOL[c.prec], i
        else:
            assert t_ref[i] - STOP32_EARLY <= t <= t_ref[i] + STOP64, (i, itm, t_ref)
            if i % 2 == 0:
                assert np.array_equal(orc.section_argmax(bm[i], c.L, c.M), idx[i]), i
