"""CPU checks of the operator's host rules through the stand-alone checker
sparc_ldpc_amd/sa_host_check (csrc/sa_host_check.cpp: sa_shape.h and
sa_tables.h only, no GPU): the k_secb chooser restated in tests/secb_cases.py
against the C++ shape rules, and the invariants of the table builders at the
smallest shapes that reach each of their branches."""
import json
import os
import subprocess

import pytest

import secb_cases as sc
from sparc_ldpc_amd._lib import SA_BACKEND_HADAMARD, SA_PREC_F32, SA_PREC_F64, plan_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
PREC = {"fp32": SA_PREC_F32, "fp64": SA_PREC_F64}
N_CUS = 256
K_SECB = 2  # SA_SEC_K_SECB


def run(*args):
    p = subprocess.run([CHECKER] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    return p.returncode, p.stdout, p.stderr


def shape(prec, L, M, n, B, plan=()):
    rc, out, err = run("shape", L, M, n, SA_BACKEND_HADAMARD, PREC[prec], plan_bits(plan), N_CUS, B)
    assert rc == 0, err
    return json.loads(out)


def assert_model_matches(prec, L, M, n, B, plan):
    want = sc.expected_instance(prec, L, M, n, B, plan)
    s = shape(prec, L, M, n, B, plan)
    secb = s["plan_of_B"][0] == K_SECB
    assert secb == (want is not None), (prec, L, M, n, B, plan, want, s)
    if want is not None:
        got = (s["E"], s["plan_of_B"][3], s["WB"], bool(s["zil"]), s["nhi"])
        assert got == (want.E, want.CB, want.W, want.ZIL, want.nhi), (prec, L, M, n, B, plan, want, s)
        assert s["CB"] == want.CB and s["plan_batched"][:2] == [s["Gb"], want.W]


def test_checker_is_built():
    assert os.path.exists(CHECKER), "sparc_ldpc_amd/sa_host_check is missing: build() makes it"
    assert run()[0] == 2 and run("shape", 1, 2)[0] == 2


@pytest.mark.parametrize("case", sc.CASES + sc.NOBANKS_CASES + sc.STOP_CASES, ids=lambda c: sc.case_id(c))
def test_model_matches_the_shape_rules_at_every_case(case):
    c = case
    assert_model_matches(c.prec, c.L, c.M, c.n, c.B, c.plan)
    s = shape(c.prec, c.L, c.M, c.n, c.B, c.plan)
    assert (s["E"], s["CB"], s["WB"], bool(s["zil"])) == (c.E, c.CB, c.W, c.ZIL)


SWEEP_N = sorted({n + d for n in sc.N_REDUCED.values() for d in (-1, 0, 1)})


@pytest.mark.parametrize("plan", [(), ("WB8",), ("WB16",), ("NO_ZIL",)], ids=lambda p: "-".join(p) or "default")
@pytest.mark.parametrize("M", [64, 128, 256, 512, 1024])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_model_matches_the_shape_rules_over_a_sweep(prec, M, plan):
    """Every CB boundary of N_REDUCED, each n and its two neighbours; a batch
    that runs k_secb where the shape has one, and one below use_batched."""
    assert len(SWEEP_N) == 18
    for n in SWEEP_N:
        assert_model_matches(prec, 19, M, n, 7, plan)
    assert_model_matches(prec, 19, M, SWEEP_N[0], 3, plan)


def test_shape_refuses_what_sa_create_refuses():
    host = 2  # SA_BACKEND_HOST: no k_secg to fall back on
    for args, msg in (((5, 48, 70000, SA_BACKEND_HADAMARD), "M not a power of two"),
                      ((4, 8192, 100, SA_BACKEND_HADAMARD), "M must be <= 4096"),
                      ((4, 64, 1 << 24, SA_BACKEND_HADAMARD), "n must be < 2^24"),
                      ((4, 64, 65535, host), "n must be < 65535"),
                      ((4, 4096, 10000, host), "does not fit in LDS")):
        rc, out, _ = run("shape", *args, SA_PREC_F64, 0, N_CUS, 1)
        d = json.loads(out)
        assert rc == 0 and d["error"] == -5 and msg in d["message"], (args, d)


def test_shape_of_a_padded_section():
    s = shape("fp32", 5, 48, 100, 1)
    assert (s["M"], s["Mu"], s["dead"], s["pow2"], s["CB"], s["G2"]) == (64, 48, 16, 0, 0, 0)


# (L, M, n, prec, plan): what the run must reach, as the checker reports it
TABLES = [
    ((11, 256, 2045, "fp32", ()), dict(E=4, banked=1, kh=2, CB=4, fwdb_lanes=16)),    # kSecbKH32
    ((11, 256, 2045, "fp64", ()), dict(E=4, banked=1, kh=2, CB=2, fwdb_lanes=16)),    # kSecbKH64
    ((19, 512, 4093, "fp32", ()), dict(E=8, WB=16, banked=1)),
    ((11, 64, 125, "fp32", ()), dict(E=1, banked=0, fwdb=1)),
    ((11, 64, sc.N_REDUCED[("fp32", 8, 2)], "fp32", ("WB8",)), dict(E=1, CB=2, banked=0, fwdb_lanes=32)),
    ((11, 256, 2045, "fp32", ("NO_BANKS",)), dict(banked=0, search=0, fwdb=1)),        # identity step order
    ((5, 48, 100, "fp32", ()), dict(M=64, dead=16, fwdb=0)),
    # SEC3 at M = 128 builds no fwd3 (k_sec43 needs k_sec4's M >= 256): the packing is reached at M = 256
    ((7, 128, 300, "fp32", ("SEC3",)), dict(sec3=0)),
    ((7, 256, 300, "fp32", ("SEC3",)), dict(sec3=1)),
    ((4, 64, 20479, "fp64", ()), dict(big=1, fwdb=0, banked=0)),                       # 32-bit inv, no pair table
]


@pytest.mark.parametrize("args,reached", TABLES, ids=["-".join(map(str, a[:4] + a[4])) for a, _ in TABLES])
def test_table_builders_keep_their_invariants(args, reached):
    L, M, n, prec, plan = args
    rc, out, err = run("tables", L, M, n, PREC[prec], plan_bits(plan))
    assert rc == 0, err
    d = json.loads(out)
    assert d["ok"] == 1
    assert {k: d[k] for k in reached} == reached, d
