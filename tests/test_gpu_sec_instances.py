"""Every one-codeword section kernel instance (csrc/sa_sec.hip: k_sec, k_secg,
k_sec2, k_sec4, k_sec43, k_sec44; 58 instances) against the oracle: one test
id per case of tests/sec_cases.py.  Each id proves through the plan report
which instance it runs, so a bad instance costs its own ids and no others.
The table is written for 256 CUs (the plan depends on the count): on another
device the ids skip."""
import numpy as np
import pytest

import sec_cases as sc
from test_gpu_parity import TOL, argmax_agree, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp(lib_gpu):
    import sparc_ldpc_amd
    return sparc_ldpc_amd


def _operator(sp, c, extra=()):
    return sp.SparcOperator(c.L, c.M, c.n, sp.make_ordering(c.L, c.M, c.n), precision=c.prec, plan=c.plan + tuple(extra))


def _plan(op, B):
    p = op.plan(B)
    return p["section_kernel"], p["row_kernel"], p["row_splits"], p["partials"]


def _held(worst, key, b, ref, c, bound, what):
    """b within `bound` of ref, with its section argmax; the error kept for the report."""
    e = rel(b, ref)
    worst[key] = max(worst.get(key, 0.0), e)
    assert e <= bound, (what, e)
    assert argmax_agree(b, ref, c.L, c.M), what


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_instance_vs_oracle(sp, case):
    c = case
    L, M, n, B, tol = c.L, c.M, c.n, c.B, TOL[c.prec]
    op = _operator(sp, c)
    if op.plan(1)["cus"] != sc.N_CUS:
        pytest.skip(f"the case table is written for {sc.N_CUS} CUs, this device has {op.plan(1)['cus']}")
    # 1. the instance (a mismatch here is a fault of the case table, not of a kernel)
    assert _plan(op, B) == (c.sec, c.row, c.rs, c.partials), op.plan(B)
    one = (c.sec, c.targ, c.row, c.rs, c.partials) if B == 1 else sc.ONE_CODEWORD[c[:6]]
    assert _plan(op, 1) == (one[0], one[2], one[3], one[4]), op.plan(1)
    assert sc.template_argument(c.sec, 1 << (M - 1).bit_length()) == c.targ  # (a padded section: 2^ceil(log2 M) columns)
    Pl = sc.flat_power(L)
    ys, refs = sc.fixed_reference(L, M, n, B)
    worst = {}

    # 2. operator products (k_sec / k_secg<E> in its product modes), before a decode
    pb, pz, pAb, pAz = sc.product_reference(L, M, n, B)
    ab0, az0 = op.Ab_batch(pb), op.Az_batch(pz)
    for i in range(B):
        worst["product"] = max(worst.get("product", 0.0), rel(ab0[i], pAb[i]), rel(az0[i], pAz[i]))
        assert rel(ab0[i], pAb[i]) <= tol and rel(az0[i], pAz[i]) <= tol, i

    # 3. the fixed-T decode (the fused tail on the k_sec4 / k_sec43 / k_sec44 + k_row2 plans)
    T = sc.T_FIXED
    bb, it = op.amp_batch(ys, Pl, T, early_stop=False)
    for i in range(B):
        _held(worst, "oracle", bb[i], refs[i], c, tol, ("fixed T", i))
    assert np.all(it == T), it
    # 4. the decisions of that decode: every section is clear (tests/test_sec_cases_host.py)
    dec = op.decide(B)
    assert np.array_equal(dec, bb.reshape(B, L, M).argmax(2))
    assert np.array_equal(dec, refs.reshape(B, L, M).argmax(2))
    # ... and the products after it: the decode's partial layouts leave them as they were
    assert np.array_equal(op.Ab_batch(pb), ab0) and np.array_equal(op.Az_batch(pz), az0)
    if c.sec in sc.MULTIWAVE:
        # the separate k_decide<E> launch and the undeferred last row step: bit for bit
        op2 = _operator(sp, c, ("NO_FUSED_TAIL",))
        assert _plan(op2, B) == _plan(op, B)
        b2, it2 = op2.amp_batch(ys, Pl, T, early_stop=False)
        assert np.array_equal(b2, bb) and np.array_equal(it2, it)
        assert np.array_equal(op2.decide(B), dec)
        del op2

    # 7. determinism: a second run, the reversed batch, each codeword alone
    b2, it2 = op.amp_batch(ys, Pl, T, early_stop=False)
    assert np.array_equal(b2, bb) and np.array_equal(it2, it)
    if B > 1:
        br, itr = op.amp_batch(ys[::-1], Pl, T, early_stop=False)
        assert np.array_equal(br[::-1], bb) and np.all(itr == T)
        for i in range(B):
            b1, it1 = op.amp_batch(ys[i:i + 1], Pl, T, early_stop=False)
            assert it1[0] == T
            _held(worst, "one", bb[i], b1[0], c, 2 * tol, ("one codeword", i))

    # 5. the beta0 start: the first step with an estimate behind it, the start's own A beta0
    b0 = sc.start_beta0(L, M, B)
    srefs = sc.start_reference(L, M, n, B)
    bs, its = op.amp_batch(ys, Pl, sc.T_START, beta0=b0, early_stop=False)
    for i in range(B):
        _held(worst, "oracle", bs[i], srefs[i], c, tol, ("beta0 start", i))
    assert np.all(its == sc.T_START), its

    # 6. the early stop on: the estimate against the oracle's after as many
    # updates as the device reports (iters = t: t updates; T: the loop ran out)
    be, ite = op.amp_batch(ys, Pl, sc.T_STOP)
    assert np.all((ite >= 1) & (ite <= sc.T_STOP)), ite
    for i in range(B):
        _held(worst, "oracle", be[i], sc.estimate_after(L, M, n, i, int(ite[i])), c, tol, ("early stop", i, int(ite[i])))
    be2, ite2 = op.amp_batch(ys, Pl, sc.T_STOP)
    assert np.array_equal(be2, be) and np.array_equal(ite2, ite)

    # 8. the report
    print(f"{sc.case_id(c)}: worst rel vs oracle {worst['oracle']:.3e} (products {worst['product']:.3e})"
          + (f", vs one-codeword decode {worst['one']:.3e}" if B > 1 else "") + f", stop indices {ite.tolist()}")
