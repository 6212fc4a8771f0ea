"""CPU checks of the k_secb case table (tests/secb_cases.py): the host model of
the chooser maps every case to its intended instance, the table covers every
selectable instance, and the oracle's decodes of the case inputs are ones a
wrong kernel could not match by accident."""
import numpy as np
import pytest

import secb_cases as sc


def test_table_covers_the_62_reachable_instances():
    assert len(sc.CASES) == 98
    assert sum(c.prec == "fp32" for c in sc.CASES) == 54 and sum(c.prec == "fp64" for c in sc.CASES) == 44
    ids = [sc.case_id(c) for c in sc.CASES + sc.NOBANKS_CASES]
    assert len(set(ids)) == len(ids)
    assert "fp32-E2-CB4-W8-zil-n253" in ids
    # the registered family (secb_lds_attrs_t): every (E, W) at CB 1 and 2
    # without ZIL, binary32 CB 4 and binary64 CB 2 with ZIL too, binary32 CB 4 without
    registered = set()
    for prec in ("fp32", "fp64"):
        for E in sc.E_ALL:
            for W in (8, 16):
                cbs = (1, 2, 4) if prec == "fp32" else (1, 2)
                for cb in cbs:
                    registered.add((prec, E, cb, W, False))
                registered.add((prec, E, 16 // sc.SIZE[prec], W, True))
    assert len(registered) == 70
    reachable = registered - set(sc.UNREACHABLE)
    assert len(sc.UNREACHABLE) == 8 and len(reachable) == 62
    assert {sc.instance_key(c) for c in sc.CASES} == reachable


@pytest.mark.parametrize("case", sc.CASES + sc.NOBANKS_CASES + sc.STOP_CASES,
                         ids=lambda c: sc.case_id(c))
def test_model_maps_case_to_its_instance(case):
    c = case
    assert c.M == 64 * c.E and c.L == c.W + 3 and c.B == (7 if c.CB > 1 else 5)
    got = sc.expected_instance(c.prec, c.L, c.M, c.n, c.B, c.plan)
    assert got is not None and got[:4] == (c.E, c.CB, c.W, c.ZIL), got
    # the tails the shape is meant to have: a second section group with 3
    # live waves, a partial last chunk, and a batch of B - 1 still batched
    assert -(-c.L // c.W) == 2 and c.L % c.W == 3
    assert c.B % c.CB != 0 or c.CB == 1
    assert sc.expected_instance(c.prec, c.L, c.M, c.n, c.B - 1, c.plan)[:4] == got[:4]
    # the default rule (no WB option) picks 16 sections per workgroup at this shape
    rest = tuple(p for p in c.plan if p not in ("WB8", "WB16"))
    assert sc.expected_instance(c.prec, c.L, c.M, c.n, c.B, rest).W == 16
    rows16 = c.CB * sc.SIZE[c.prec] == 16
    if "NO_BANKS" in c.plan:
        assert rows16 and c.E in (4, 8) and not got.banked and not got.GS and got.nhi == 8
    elif rows16 and c.n == 2 * c.M - 3:
        assert got.nhi == 2 and not got.GS and got.banked == (c.E >= 4)  # the general loop, a short KH block
    elif rows16 and c.n == 8 * c.M - 3:
        assert got.nhi == 8 and got.banked == got.GS == (c.E >= 4)       # the sign-split loop
    else:
        assert not got.banked and not got.GS


def test_reduced_cb_n_is_the_first_odd_n_past_the_larger_cb():
    for (prec, W, cb), n in sc.N_REDUCED.items():
        for E in (1, 2, 4, 8):
            M = 64 * E
            assert n % 2 == 1
            assert sc.cb_for(prec, M, n, W)[0] == cb and sc.cb_for(prec, M, n - 2, W)[0] == 2 * cb, (prec, W, cb, E)


def test_e16_sixteen_byte_rows_are_unreachable():
    """No (n, plan) selects E = 16 with 16-byte rows; L and B do not enter cb_for."""
    for prec, E, CB, W, zil in sc.UNREACHABLE:
        s = sc.SIZE[prec]
        assert W * 1024 * CB * s > (sc.LDS_FULL if W == 16 else sc.LDS_HALF)
        for n in list(range(1, 4096)) + list(range(4096, sc.LDS_FULL // s + 64, 61)):
            for plan in (("WB8",), ("WB16",), (), ("WB8", "NO_ZIL"), ("WB16", "NO_ZIL")):
                got = sc.expected_instance(prec, W + 3, 1024, n, 8, plan)
                assert got is None or got.CB * s != 16, (prec, n, plan, got)


def test_default_rule_never_selects_w8():
    for prec in ("fp32", "fp64"):
        for E in sc.E_ALL:
            for n in list(range(1, 2048, 7)) + list(range(2048, sc.LDS_FULL // sc.SIZE[prec] + 64, 97)):
                got = sc.expected_instance(prec, 19, 64 * E, n, 8, ())
                assert got is None or got.W == 16, (prec, E, n, got)


SHAPES = sorted({(c.L, c.M, c.n, c.B) for c in sc.CASES + sc.NOBANKS_CASES})


def test_fifty_shapes():
    assert len(SHAPES) == 50


@pytest.mark.parametrize("L,M,n,B", SHAPES)
def test_oracle_keeps_the_gpu_test_sharp(L, M, n, B):
    """Conditions on the inputs, not tolerances: after T = 3 iterations at
    capacity-rate noise most sections are neither still flat nor saturated
    (an error anywhere in the section step moves the estimate), and every
    section's argmax is clear at argmax_agree's margin, so the argmax
    comparison leaves no section out.  Measured: smallest unsaturated share
    0.73, every shape fully clear."""
    ys, refs = sc.fixed_reference(L, M, n, B)
    assert ys.shape == (B, n) and refs.shape == (B, L * M)
    r = refs.reshape(B * L, M)
    top = r.max(1) / np.sqrt(n * sc.P / L)
    share = np.mean((top > 0.02) & (top < 0.98))
    srt = np.sort(r, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-5 * np.maximum(srt[:, -1], 1e-300)
    print(f"L={L} M={M} n={n} B={B}: unsaturated share {share:.3f}, clear {clear.mean():.3f}")
    assert share >= 0.5
    assert clear.all()


STOP_SHAPES = sorted({(c.L, c.M, c.n, c.B) for c in sc.STOP_CASES})


@pytest.mark.parametrize("L,M,n,B", STOP_SHAPES)
def test_oracle_stop_indices_are_mixed(L, M, n, B):
    """Every even codeword (rho = 0.35) stops at least 3 iterations before
    each odd one (rho = 1): a chunk then holds frozen and live codewords."""
    idx, ys, refs, ts, _ = sc.stop_reference(L, M, n, B)
    print(f"L={L} M={M} n={n} B={B}: oracle stop indices {ts.tolist()}")
    assert ts[0::2].max() + 3 <= ts[1::2].min(), ts
    for i in range(0, B, 2):  # the oracle decodes every even codeword correctly
        assert np.array_equal(refs[i].reshape(L, M).argmax(1), idx[i])
