"""CPU check of the packed tables of the pair / quad section kernels (k_sec4,
k_sec44; csrc/sa_tables.h: pack_inv_section, pack_fwd_pair) through the
stand-alone checker's `packed` subcommand: both tables are built from inv and
fwd2 as build_tables builds them, unpacked on the host and compared entry for
entry; the rule that asks for them (csrc/sa_shape.h: Shape::pack_inv,
pack_fwd) is read from the same report."""
import json
import os
import subprocess

import pytest

from sparc_ldpc_amd._lib import SA_PREC_F32, SA_PREC_F64, plan_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "sa_host_check")
PREC = {"fp32": SA_PREC_F32, "fp64": SA_PREC_F64}

# (M, n): nhi = 2; c2's section shape; one row into a fourth pass of the row
# phase (4608 rows per pass: a second set of words); the largest packable row
# index, nhi = 32, two blocks of 16 bucket steps; a small M = 256 shape
SHAPES = [(512, 1021), (512, 4608), (512, 4609), (256, 8190), (256, 509)]


def packed(L, M, n, prec="fp32", plan=()):
    p = subprocess.run([CHECKER, "packed"] + [str(a) for a in (L, M, n, PREC[prec], plan_bits(plan))],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout)


def ilog2(x):
    return (x - 1).bit_length()


@pytest.mark.parametrize("L", [257, 255])  # odd: the last pair has one section
@pytest.mark.parametrize("M,n", SHAPES)
def test_packed_tables_unpack_to_inv_and_fwd2(M, n, L):
    d = packed(L, M, n)
    w = 1 << ilog2(max(M + 1, n + 1))
    nhi, EQ = w // M, M // 256
    assert (d["ok"], d["pack_inv"], d["pack_fwd"], d["kh"], d["nhi"]) == (1, 1, 1, 16, nhi)
    # a record: EQ x 16 entries of 13 bits in whole dwords; blocks of 16 steps; words of three rows
    rd, blocks, words = (EQ * 16 * 13 + 31) // 32, (nhi + 15) // 16, 3 * ((n + 4607) // 4608)
    assert (d["rd"], d["blocks"], d["words"]) == (rd, blocks, words)
    assert d["invp_bytes"] == L * 4 * blocks * 64 * rd * 4
    assert d["fwd2p_bytes"] == (L + 1) // 2 * words * 512 * 8
    assert d["inv_bytes"] == L * w * 2 and d["fwd2_bytes"] == (L + 1) // 2 * n * 4


def test_c2_record_and_bytes():
    """c2's section shape: 13 dwords per lane and block against 16, three
    8-byte words against nine 4-byte entries."""
    d = packed(257, 512, 4608)
    assert d["rd"] == 13 and d["words"] == 3
    assert d["invp_bytes"] * 16 == d["inv_bytes"] * 13
    assert d["fwd2p_bytes"] * 3 == d["fwd2_bytes"] * 2


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_quads_pack_the_bucket_table_alone(prec):
    """SEC4Q reads the pair table with 1024-thread passes and keeps it; the
    binary64 quads gather in blocks of 8 bucket steps, and so do their records."""
    d = packed(257, 256, 8190, prec, ("SEC4Q",))
    kh = 8 if prec == "fp64" else 16
    assert (d["pack_inv"], d["pack_fwd"], d["kh"], d["blocks"]) == (1, 0, kh, 32 // kh)
    assert d["rd"] == (kh * 13 + 31) // 32


def test_rule_edges():
    assert packed(255, 256, 8190)["pack_inv"] == 1                # n + 1 < 8192
    d = packed(255, 256, 8191)
    assert (d["ok"], d["pack_inv"], d["pack_fwd"]) == (1, 0, 0)    # ... and the first n past it
    for prec in ("fp32", "fp64"):                                 # either precision
        assert packed(257, 512, 1021, prec)["pack_inv"] == 1
    d = packed(257, 1024, 2045)                                   # M <= 512
    assert (d["pack_inv"], d["pack_fwd"]) == (0, 0)
    d = packed(257, 512, 1021, plan=("SEC3",))                    # triples keep their own tables
    assert (d["pack_inv"], d["pack_fwd"]) == (0, 0)
    assert packed(257, 128, 253)["pack_inv"] == 0                 # k_sec2
    d = packed(257, 512, 1021, plan=("NO_PACK",))
    assert (d["pack_inv"], d["pack_fwd"], d["invp_bytes"], d["fwd2p_bytes"]) == (0, 0, 0, 0)


def test_existing_subcommands_do_not_know_the_option_as_a_shape_field():
    """NO_PACK is a valid plan option of `shape`, whose report keeps its fields."""
    p = subprocess.run([CHECKER, "shape", "257", "512", "1021", "0", "0", str(plan_bits(("NO_PACK",))), "256", "1"],
                       capture_output=True, text=True, timeout=60)
    d, d0 = json.loads(p.stdout), json.loads(subprocess.run(
        [CHECKER, "shape", "257", "512", "1021", "0", "0", "0", "256", "1"], capture_output=True, text=True,
        timeout=60).stdout)
    assert "error" not in d and set(d) == set(d0) and not any("pack" in k for k in d)
    assert {k: v for k, v in d.items() if k != "plan"} == {k: v for k, v in d0.items() if k != "plan"}
