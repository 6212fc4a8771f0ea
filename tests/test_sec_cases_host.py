"""CPU checks of the one-codeword section kernels' case table
(tests/sec_cases.py): every row's literal plan is what the shape rules of
csrc/sa_shape.h report (sparc_ldpc_amd/sa_host_check, 256 CUs), the table
covers all 58 registered instances, a sweep over n establishes where k_sec2
can be selected at all, the fast form of the oracle's transforms is the
oracle's bit for bit, and the oracle's decodes of the case inputs are ones a
wrong kernel could not match by accident."""
import json
import os
import subprocess

import numpy as np
import pytest

import sec_cases as sc
from oracle import amp_oracle as orc
from sparc_ldpc_amd._lib import SA_BACKEND_HADAMARD, SA_PREC_F32, SA_PREC_F64, plan_bits
from sparc_ldpc_amd.operators import SparcOperator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
PREC = {"fp32": SA_PREC_F32, "fp64": SA_PREC_F64}
SEC, ROW = SparcOperator.SECTION_KERNELS, SparcOperator.ROW_KERNELS  # sa_plan's numbers
LDS = 160 * 1024


def run(*args):
    p = subprocess.run([CHECKER] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


def shape(c, B):
    return run("shape", c.L, c.M, c.n, SA_BACKEND_HADAMARD, PREC[c.prec], plan_bits(c.plan), sc.N_CUS, B)


def reported(s):
    """(section kernel, template argument, row kernel, row splits, partials) of a checker report."""
    sec, G, rs, _, _, _, row, cus = s["plan_of_B"]
    assert cus == sc.N_CUS
    return SEC[sec], sc.template_argument(SEC[sec], s["M"]), ROW[row], rs, G


@pytest.mark.parametrize("case", sc.CASES + sc.HOST_CASES, ids=sc.case_id)
def test_case_is_what_the_shape_rules_report(case):
    c = case
    s = shape(c, c.B)
    assert reported(s) == (c.sec, c.targ, c.row, c.rs, c.partials), s
    assert (s["big"] == 1) == (c.sec == "k_secg")
    assert s["dead"] == (16 if c.M == 48 else 0) and s["E"] == sc.template_argument("k_sec", s["M"])
    # the one-codeword decode of the same operator, which the GPU test compares with
    one = reported(shape(c, 1))
    assert one == ((c.sec, c.targ, c.row, c.rs, c.partials) if c.B == 1 else sc.ONE_CODEWORD[c[:6]]), one
    # the tails the shape is meant to have
    if c.sec in sc.MULTIWAVE:
        per = {"k_sec2": 2, "k_sec4": 2, "k_sec43": 3, "k_sec44": 4}[c.sec]
        assert c.partials == -(-c.L // per) and c.rs == 1
        assert c.L % per != 0 or c.B > 1  # one codeword: the last workgroup is short of a section
    else:
        assert c.partials == -(-c.L // 4)
    if c.n == 2 * c.M - 3:
        assert s["nhi"] == 2 and s["w"] == 2 * c.M


def test_ids_are_unique_and_b_gt_1_rows_have_their_one_codeword_plan():
    ids = [sc.case_id(c) for c in sc.CASES + sc.HOST_CASES]
    assert len(set(ids)) == len(ids)
    assert {c[:6] for c in sc.CASES if c.B > 1} == set(sc.ONE_CODEWORD)
    assert all(c.gpu for c in sc.CASES) and not any(c.gpu for c in sc.HOST_CASES)


def test_table_covers_the_58_registered_instances():
    registered = {(k, a, prec) for k, args in sc.REGISTERED.items() for a in args for prec in ("fp32", "fp64")}
    assert len(registered) == 58
    # the instance of a case: from the section kernel the checker reports and M,
    # as launch_sec / launch_sec2 switch on them
    ran = set()
    for c in sc.CASES:
        sec, targ = reported(shape(c, c.B))[:2]
        ran.add((sec, targ, c.prec))
    missing = registered - ran
    assert not missing, sorted(missing)
    assert ran == registered
    assert ran == {sc.instance_key(c) for c in sc.CASES}
    # a decode on a multi-wave kernel takes its products, its beta0 start and
    # its k_decide through k_sec<E> of the same section size
    assert len(sc.CASES) == 86 and len(sc.HOST_CASES) == 4


def sweep(prec, M, L=257, B=1, n1=70000):
    runs = run("sweep", L, M, SA_BACKEND_HADAMARD, PREC[prec], 0, sc.N_CUS, B, 1, n1)
    assert runs[0][0] == 1 and runs[-1][1] == n1
    assert all(a[1] + 1 == b[0] for a, b in zip(runs, runs[1:]))
    return [(lo, hi, SEC[sec] if sec >= 0 else None, big) for lo, hi, sec, big in runs]


@pytest.mark.parametrize("M", [128, 256, 512, 1024, 2048, 4096])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_sweep_of_n_where_each_kernel_is_selected(prec, M):
    """Every n from 1 to 70000 (past each LDS limit and the 16-bit rows) at
    L = 257, one codeword, the default plan: k_sec4, then k_sec2 for exactly
    16 values of n, then k_sec for 12, then k_secg; at M = 128 (no k_sec4)
    k_sec2 up to its LDS limit.  No multi-wave kernel where `big` is set."""
    runs = sweep(prec, M)
    s = 4 if prec == "fp32" else 8
    for lo, hi, sec, big in runs:
        assert sec is not None
        assert (sec == "k_secg") == bool(big), (lo, hi, sec, big)
        assert not (big and sec in sc.MULTIWAVE)
    kernels = [r[2] for r in runs]
    sec2 = [(lo, hi) for lo, hi, sec, _ in runs if sec == "k_sec2"]
    assert len(sec2) == 1
    lo, hi = sec2[0]
    if M == 128:
        assert kernels == ["k_sec2", "k_sec", "k_secg"] and lo == 1
    else:
        assert kernels == ["k_sec4", "k_sec2", "k_sec", "k_secg"]
        assert (lo, hi) == (sc.SEC2_WINDOW[(M, prec)], sc.SEC2_WINDOW[(M, prec)] + 15)
    # the window's end is k_sec2's LDS limit: (n + 1) s rounded to 16 bytes, 4 M s of T and exchange, 16 s
    assert ((hi + 1) * s + 15) // 16 * 16 + 4 * M * s + 16 * s <= LDS < ((hi + 2) * s + 15) // 16 * 16 + 4 * M * s + 16 * s
    k_sec = [(a, b) for a, b, sec, _ in runs if sec == "k_sec"][0]
    assert k_sec == (hi + 1, hi + 12)
    assert runs[-1][0] == hi + 13 and runs[-1][2] == "k_secg"
    print(f"{prec} M={M}: " + ", ".join(f"{sec} n={a}..{b}" for a, b, sec, _ in runs))


def test_fp64_m4096_ladder():
    """All four kernels within 30 rows, each rung a case of the table."""
    assert sweep("fp64", 4096) == [(1, 4063, "k_sec4", 0), (4064, 4079, "k_sec2", 0), (4080, 4091, "k_sec", 0),
                                   (4092, 70000, "k_secg", 1)]
    rungs = {c.n: c.sec for c in sc.CASES if c.prec == "fp64" and (c.L, c.M, c.B) == (257, 4096, 1)}
    assert rungs == {4061: "k_sec4", 4063: "k_sec4", 4064: "k_sec2", 4079: "k_sec2", 4080: "k_sec", 4092: "k_secg"}


def test_k_secg_cases_sit_on_the_first_odd_n_past_the_lds():
    for c in sc.CASES:
        if c.sec == "k_secg" and c.L == 5 and c.n < 65535:
            runs = sweep(c.prec, c.M, L=5)
            assert [r[2] for r in runs] == ["k_sec", "k_secg"]
            first = runs[1][0]
            odd = first + (1 - first % 2)
            assert c.n % 2 == 1 and (odd, c.n) == sc.K_SECG_MOVED.get((c.prec, c.M), (odd, odd)), (c, first)
    assert sum(c.sec == "k_secg" and c.n >= 65535 for c in sc.CASES) == 2


def test_row_kernels_have_a_partial_last_block():
    """n odd, or no multiple of 16, except where a case sits on a boundary of
    the rules that is one (the k_sec2 windows begin at multiples of 16)."""
    on_boundary = set(sc.SEC2_WINDOW.values()) | {v + 16 for v in sc.SEC2_WINDOW.values()}
    for c in sc.CASES:
        assert c.n % 16 != 0 or c.n in on_boundary, c


FAST_SHAPES = [(5, 64, 125), (9, 48, 125), (7, 128, 300), (6, 256, 509), (3, 1024, 2045), (3, 256, 5000), (2, 4096, 4061),
               (33, 256, 39904), (5, 64, 65537)]  # w = 65536 and 131072: 8 and 11 stages above M


@pytest.mark.parametrize("L,M,n", FAST_SHAPES)
def test_fast_transforms_are_the_oracles_bit_for_bit(L, M, n):
    Ab, Az, ordering = sc.fast_transforms(L, M, n)
    oAb, oAz, oord = orc.sparc_transforms(L, M, n)
    assert np.array_equal(ordering, oord)
    rs = np.random.RandomState(L + M + n)
    for _ in range(2):
        b, z = rs.randn(L * M, 1), rs.randn(n, 1)
        assert np.array_equal(Ab(b), oAb(b)) and np.array_equal(Az(z), oAz(z))
    onehot = np.zeros((L * M, 1))
    onehot[np.arange(L) * M + rs.randint(0, M, L), 0] = 1.5
    assert np.array_equal(Ab(onehot), oAb(onehot))
    # and with them the whole loop
    Pl = sc.flat_power(L)
    y = orc.rep_inputs(L, M, n, Pl, sc.sigma_at(L, M, n), oAb, 50)[1]
    assert np.array_equal(sc.inputs(L, M, n, 1)[0], y.reshape(-1))
    assert np.array_equal(sc.fixed_reference(L, M, n, 1)[1][0],
                          orc._amp_core(y, Pl, L, M, sc.T_FIXED, oAb, oAz, None, early_stop=False)[0].reshape(-1))


SHAPES = sorted({sc.shape_of(c) + (max(d.B for d in sc.CASES if sc.shape_of(d) == sc.shape_of(c)),) for c in sc.CASES})


@pytest.mark.parametrize("L,M,n,B", SHAPES)
def test_oracle_keeps_the_gpu_test_sharp(L, M, n, B):
    """Conditions on the inputs, not tolerances: after T = 3 iterations at
    capacity-rate noise at least half of the sections are neither still flat
    nor saturated (an error anywhere in the section step moves the estimate),
    and every section's argmax is clear at argmax_agree's margin, so the
    argmax comparison and the comparison of decisions leave no section out."""
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
