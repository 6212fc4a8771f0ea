"""CPU checks of the LDPC decoder's host rules (csrc/ldpc_plan.h through
sparc_ldpc_amd/lb_host_check): the four LDPC case tables' plan columns are what
the rules report, every boundary of the rules on tiny synthetic graphs with the
expected value from the rule's own inequality, the measurement switches, every
refusal with its code and message, the tail's grids by hand, and the graph
tables against NumPy."""
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import ldpc_cases as lc
import ldpc_f32_cases as fc
import ldpc_fixed_cases as qc
import ldpc_layered_cases as llc
import ldpc_layered_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKER = os.path.join(ROOT, "sparc_ldpc_amd", "lb_host_check")
LDS = 160 * 1024 - 64  # 163776: what a workgroup's dynamic LDS may take
SUMPROD2, SUMPROD, MINSUM, L_SUMPROD2, L_MINSUM, F32, FIXED = 0, 1, 2, 3, 4, 0x100, 0x400
ARG, GRAPH, UNSUPPORTED = -1, -4, -5


def run(cmd, *args, stdin="", status=0, **switches):
    words = [str(a) for a in args] + [f"LDPC_BP_{k}={v}" for k, v in switches.items()]
    p = subprocess.run([CHECKER, cmd] + words, input=stdin, capture_output=True, text=True, timeout=120)
    assert p.returncode == status, (p.returncode, p.stderr)
    return json.loads(p.stdout) if status == 0 else None


def plan(graph, *args, layers=None, **kw):
    """graph: (vdeg, cdeg, intrlv); layers: first_check, or None for no layers."""
    vdeg, cdeg, intrlv = (np.asarray(a, dtype=np.int64) for a in graph)
    first = [] if layers is None else list(layers)
    head = [len(vdeg), len(cdeg), len(intrlv), max(len(first) - 1, 0)]
    return run("plan", *args, stdin=" ".join(map(str, head + list(vdeg) + list(cdeg) + list(intrlv) + first)), **kw)


def refused(out, code, fragment):
    assert set(out) == {"error", "message"} and out["error"] == code and fragment in out["message"], out
    return True


# ---- the case tables against the rules -------------------------------------------------

@functools.lru_cache(maxsize=None)
def cell_plan(cell):
    """The checker's report of a cell's code with its protograph layers, at the default widths, resolved
    for the binary32 layered sumprod2 type."""
    c = (llc if cell in llc.CELLS else lc).make_code(cell)
    return c, plan((c.vdeg, c.cdeg, c.intrlv), 2, 6, 8, L_SUMPROD2 | F32, 0.0, 10, 0, layers=lr.code_layers(c))


@pytest.mark.parametrize("cell", list(lc.CELLS))
def test_flooding_cells(cell):
    c, p = cell_plan(cell)
    g = p["graph"]
    max_cdeg, max_vdeg, lds, fixed_dc, threads = lc.CELLS[cell][1]
    assert (g["Nv"], g["Nc"], g["Nmsg"]) == (c.Nv, c.Nc, c.Nmsg)
    assert (g["maxdc"], g["lds"], g["maxdc"] if g["fixed"] else 0, g["nt"]) == (max_cdeg, lds, fixed_dc, threads), g
    assert max_vdeg is None or g["maxdv"] == max_vdeg
    assert g["tail_at"] == g["tail_default"] == (0 if cell == "syn_dv13" else 8)
    assert g["dcmax"] == (8 if max_cdeg <= 8 else 16 if max_cdeg <= 16 else 32)


@pytest.mark.parametrize("cell", list(llc.CELLS))
def test_layered_cells(cell):
    c, p = cell_plan(cell)
    l = p["layers"]
    assert (l["lmode"], l["maxlayer"], l["lnt"]) == llc.CELLS[cell][1], l
    assert l["nlayers"] == c.Nc // c.z


@pytest.mark.parametrize("cell", list(fc.CELLS))
def test_f32_cells(cell):
    c, p = cell_plan(cell)
    l, s = p["layers"], p["launch"]
    assert (l["lmode32"], l["maxlayer"], l["lnt"], s["shm"]) == fc.CELLS[cell][:4], (l, s)
    assert p["type"]["f32"] == 1 and p["type"]["hbm"] == (l["lmode32"] < 2) and (s["mode"], s["nt"]) == (l["lmode32"], l["lnt"])
    assert (s["dcmax"], s["dcfix"]) == ((32, 20) if l["lfixed"] else (p["graph"]["dcmax"], 0))


@pytest.mark.parametrize("cell", list(qc.CELLS))
def test_fixed_cells(cell):
    c, p = cell_plan(cell)
    q = p["fixed"]
    assert (q["qnt"], q["qlanes"]) == qc.CELLS[cell], q
    assert q["qlds"] == qc.lds_bytes(c) and q["qfit"] == 1 and (q["qfrac"], q["qmsg"], q["qapp"]) == (2, 6, 8)
    # the instance the fixed-point type launches: lanes x ceil(degree class / lanes) edges a lane
    s = plan((c.vdeg, c.cdeg, c.intrlv), 2, 6, 8, L_MINSUM | FIXED, 0.75, 10, 0, layers=lr.code_layers(c))["launch"]
    dc = int(c.cdeg.max())
    cls = 8 if dc <= 8 else 16 if dc <= 16 else 20 if dc <= 20 else 32
    assert (s["nt"], s["shm"], s["lanes"], s["dcmax"], s["epl"]) == (q["qnt"], q["qlds"], q["qlanes"], cls, -(-cls // q["qlanes"]))


# ---- boundaries, on tiny synthetic graphs ----------------------------------------------

def checks(total, d=8):
    """Check degrees of sum `total`: checks of degree d and one for the rest."""
    return [d] * (total // d) + ([total % d] if total % d else [])


def graph(cdeg, vdeg=None):
    """A valid graph on the given degrees (every variable of degree 1 unless vdeg is given); port p
    of the variables, in order, is message p of the checks."""
    n = sum(cdeg)
    vdeg = [1] * n if vdeg is None else vdeg
    assert sum(vdeg) == n
    return vdeg, cdeg, np.arange(n)


def one_layer(cdeg):
    return [0, len(cdeg)]


def test_lds_flips_at_20472_messages():
    # Nmsg * 8 <= 163776
    assert 20472 * 8 == LDS
    assert plan(graph(checks(20472)))["graph"]["lds"] == 1
    assert plan(graph(checks(20473)))["graph"]["lds"] == 0


@pytest.mark.parametrize("Nc,nt", [(256, 256), (257, 320), (1025, 1024)])
def test_flooding_threads(Nc, nt):
    # a thread per check, in whole waves, at least 256 and at most 1024
    assert plan(graph([2] * Nc))["graph"]["nt"] == nt


def test_variable_degree_12_and_13():
    g = plan(graph([2] * 8, [12] + [1] * 4))["graph"]
    assert (g["maxdv"], g["nq"], g["tail_at"]) == (12, 3, 8)
    g = plan(graph([2] * 8, [13] + [1] * 3))["graph"]
    assert (g["maxdv"], g["nq"], g["tail_at"], g["tail_default"]) == (13, 0, 0, 0)
    assert [plan(graph([2] * 8, [dv] + [1] * (16 - dv)))["graph"]["nq"] for dv in (1, 4, 5, 8, 9)] == [1, 1, 2, 2, 3]


def test_check_regular_degree_20():
    # the straight-line instance: every check of degree 20, and at most 768 threads
    g = plan(graph([20] * 768))["graph"]
    assert (g["nt"], g["fixed"], g["dcmax"]) == (768, 1, 32)
    g = plan(graph([20] * 769))["graph"]
    assert (g["nt"], g["fixed"]) == (832, 0)
    g = plan(graph([20] * 767 + [19]))["graph"]
    assert (g["nt"], g["fixed"], g["mindc"]) == (768, 0, 19)
    # the layered instances keep it past 768 checks (their bound is on the layer's threads)
    assert plan(graph([20] * 769), layers=[0, 769])["layers"]["lfixed"] == 1
    assert plan(graph([20] * 767 + [19]), layers=[0, 768])["layers"]["lfixed"] == 0


def test_degree_classes():
    for dc, cls in [(8, 8), (9, 16), (16, 16), (17, 32), (32, 32)]:
        assert plan(graph([dc, 2]))["graph"]["dcmax"] == cls
    for dc, cls in [(8, 8), (9, 16), (16, 16), (17, 20), (20, 20), (21, 32)]:
        s = plan(graph([dc, 2]), 2, 6, 8, L_MINSUM | FIXED, 0.75, 10, 0, layers=[0, 1, 2])["launch"]
        assert (s["dcmax"], s["epl"]) == (cls, -(-cls // s["lanes"]))


def test_layered_modes_on_each_side_of_the_lds():
    # (Nv + Nmsg) * el <= 163776: r and app in LDS; Nv * el <= 163776: app alone.  Nv = Nmsg here.
    def modes(n):
        l = plan(graph(checks(n, 32)), layers=[0, len(checks(n, 32))])["layers"]
        return l["lmode"], l["lmode32"]
    assert 2 * 10236 * 8 == LDS and 20472 * 8 == LDS and 2 * 20472 * 4 == LDS and 40944 * 4 == LDS
    assert modes(10236) == (2, 2) and modes(10237) == (1, 2)
    assert modes(20472) == (1, 2) and modes(20473) == (0, 1)
    assert modes(40944) == (0, 1) and modes(40945) == (0, 0)


def test_layered_threads():
    # a thread per edge of the largest layer, at least 128, at most 1024 (768 with the degree-20 instances)
    l = plan(graph([8] * 8), layers=[0, 8])["layers"]
    assert (l["maxedges"], l["lnt"]) == (64, 128)
    l = plan(graph([8] * 480 + [8] * 3), layers=[0, 480, 483])["layers"]
    assert (l["maxlayer"], l["maxedges"], l["lnt"], l["lfixed"]) == (480, 3840, 1024, 0)
    l = plan(graph([20] * 192 + [20] * 3), layers=[0, 192, 195])["layers"]
    assert (l["maxlayer"], l["maxedges"], l["lnt"], l["lfixed"]) == (192, 3840, 768, 1)
    l = plan(graph([8] * 25), layers=[0, 25])["layers"]
    assert (l["maxedges"], l["lnt"]) == (200, 256)


@pytest.mark.parametrize("maxdc,lanes", [(1, 1), (2, 2), (3, 2), (31, 16), (32, 16)])
def test_fixed_lanes_capped_by_the_check_degree(maxdc, lanes):
    # the largest power of two <= min(maxdc, 16); one check a layer leaves the thread bound out of it
    assert plan(graph([maxdc]), layers=[0, 1])["fixed"]["qlanes"] == lanes


def test_fixed_lanes_and_threads():
    def fixed(nchecks):
        return plan(graph([16] * nchecks), layers=[0, nchecks])["fixed"]
    # lanes double while maxlayer * lanes * 2 <= 768: 48 * 8 * 2 = 768, 49 * 8 * 2 = 784
    q = fixed(48)
    assert (q["qlanes"], q["qnt"]) == (16, 1024)  # 768 threads: over a third of 2048
    q = fixed(49)
    assert (q["qlanes"], q["qnt"]) == (8, 448)  # 392 in whole waves
    # nt * 3 > 2048 takes all 1024 threads: 640 * 3 = 1920, 704 * 3 = 2112
    assert (fixed(40)["qlanes"], fixed(40)["qnt"]) == (16, 640)
    assert (fixed(44)["qlanes"], fixed(44)["qnt"]) == (16, 1024)
    assert fixed(1)["qnt"] == 64


def test_fixed_image_on_each_side_of_the_lds():
    # 2 Nv + Nmsg rounded up to 16 <= 163776; Nv = Nmsg
    assert 3 * 54592 == LDS
    for n, lds, fit in [(54592, LDS, 1), (54593, LDS + 16, 0)]:
        g = graph(checks(n, 32))
        q = plan(g, layers=one_layer(g[1]))["fixed"]
        assert (q["qlds"], q["qfit"]) == (lds, fit)
    out = plan(g, 2, 6, 8, L_MINSUM | FIXED, 0.75, 10, 0, layers=one_layer(g[1]))
    assert refused(out, UNSUPPORTED, "the image (163792 bytes) does not fit a workgroup's LDS")


# ---- switches ------------------------------------------------------------------------------

SMALL = graph([8] * 8)  # lmode 2 in both precisions, 64 edges in its one layer
REG20 = graph([20] * 8)


def test_switch_layered_lds():
    for v, mode in [(0, 0), (1, 1), (2, 2), (3, 2), (-1, 0)]:
        l = plan(SMALL, layers=[0, 8], LAYERED_LDS=v)["layers"]
        assert (l["lmode"], l["lmode32"]) == (mode, mode), v
    assert plan(SMALL, layers=[0, 8], LAYERED_LDS="")["layers"]["lmode"] == 2


def test_switch_layered_threads():
    for v, nt, nt20 in [(100, 64, 64), (192, 192, 192), (5000, 1024, 768), (0, 64, 64)]:
        assert plan(SMALL, layers=[0, 8], LAYERED_THREADS=v)["layers"]["lnt"] == nt
        assert plan(REG20, layers=[0, 8], LAYERED_THREADS=v)["layers"]["lnt"] == nt20


def test_switch_f32_resident():
    args = (2, 6, 8, L_MINSUM | F32, 0.75, 10, 0)
    p = plan(SMALL, *args, layers=[0, 8], LAYERED_F32_RESIDENT=1)
    assert p["layers"]["lone32"] == 1 and p["launch"]["shm"] == 80 * 1024 + 64  # more than half of the LDS
    p = plan(SMALL, *args, layers=[0, 8], LAYERED_F32_RESIDENT=2)
    assert p["layers"]["lone32"] == 0 and p["launch"]["shm"] == 4 * (64 + 64)
    p = plan(SMALL, 2, 6, 8, L_MINSUM, 0.75, 10, 0, layers=[0, 8], LAYERED_F32_RESIDENT=1)
    assert p["launch"]["shm"] == 8 * (64 + 64)  # binary32 alone


def test_switch_fixed_lanes_and_threads():
    assert plan(SMALL, layers=[0, 8])["fixed"]["qlanes"] == 8
    assert plan(SMALL, layers=[0, 8], FIXED_LANES=3)["fixed"]["qlanes"] == 8  # not a power of two: ignored
    q = plan(SMALL, layers=[0, 8], FIXED_LANES=16)["fixed"]
    assert (q["qlanes"], q["qnt"]) == (16, 128)
    q = plan(REG20, layers=[0, 8], FIXED_LANES=8)["fixed"]
    assert (q["qlanes"], q["qnt"]) == (8, 64)
    assert plan(SMALL, layers=[0, 8], FIXED_THREADS=130)["fixed"]["qnt"] == 128
    assert plan(SMALL, layers=[0, 8], FIXED_THREADS=5000)["fixed"]["qnt"] == 1024
    assert plan(SMALL, layers=[0, 8], FIXED_THREADS=10)["fixed"]["qnt"] == 64


def test_switch_tail():
    for v, at in [(5, 5), (0, 0), ("", 8), (-3, 0)]:
        g = plan(SMALL, TAIL=v)["graph"]
        assert (g["tail_at"], g["tail_default"]) == (at, at), v
    assert plan(graph([2] * 8, [13] + [1] * 3), TAIL=5)["graph"]["tail_at"] == 0  # no tail past degree 12


def test_malformed_command_lines():
    run("plan", 2, 6, stdin="1 1 1 0 1 1 0", status=2)
    run("plan", "BOGUS=1", stdin="1 1 1 0 1 1 0", status=2)
    run("plan", stdin="4 1 4 0 1 1", status=2)  # the input ends early
    run("tail", 8, 3, 1, status=2)
    run("nothing", status=2)


# ---- refusals --------------------------------------------------------------------------------

def test_graph_refusals():
    assert refused(plan(([], [], [])), ARG, "empty or null graph")
    assert refused(plan(([2, -1, 1], [2], [0, 1])), GRAPH, "negative variable degree")
    assert refused(plan(([1, 1], [2, 0], [0, 1])), GRAPH, "check node of degree < 1")
    assert refused(plan(([1, 1], [3], [0, 1])), GRAPH, "sum(vdeg) and sum(cdeg) must equal Nmsg")
    assert refused(plan(([1, 2], [2], [0, 1])), GRAPH, "sum(vdeg) and sum(cdeg) must equal Nmsg")
    assert refused(plan(([1] * 40, [40], np.arange(40))), UNSUPPORTED, "check degree > 32")
    assert refused(plan(([256], [32] * 8, np.arange(256))), UNSUPPORTED, "variable degree > 255")
    for il in ([0, 0], [0, 2], [-1, 0]):
        assert refused(plan(([1, 1], [2], il)), GRAPH, "intrlv is not a permutation")
    assert plan(([255, 1], [32] * 8, np.arange(256)))["graph"]["maxdv"] == 255


def test_layer_refusals():
    g = graph([2, 2, 2, 2])
    assert plan(g, layers=[0, 1, 2, 3, 4])["layers"]["nlayers"] == 4
    stdin = "8 4 8 -1  1 1 1 1 1 1 1 1  2 2 2 2  0 1 2 3 4 5 6 7"  # nlayers < 1
    assert refused(run("plan", stdin=stdin), ARG, "bad layer arguments")
    assert refused(plan(g, layers=[1, 2, 4]), GRAPH, "first_check[0] must be 0")
    assert refused(plan(g, layers=[0, 2, 2, 4]), GRAPH, "first_check must increase strictly from 0 to Nc (layer 1)")
    assert refused(plan(g, layers=[0, 2, 5]), GRAPH, "first_check must increase strictly from 0 to Nc (layer 1)")
    assert refused(plan(g, layers=[0, 1, 3]), GRAPH, "first_check[nlayers] = 3 is not Nc = 4")
    g2 = graph([2, 2], [2, 1, 1])  # variable 0 fills check 0
    assert refused(plan(g2, layers=[0, 2]), GRAPH, "layer 0: variable 0 occurs twice")
    g3 = graph([2, 2, 2], [1, 1, 1, 2, 1])  # variable 3 in checks 1 and 2
    assert refused(plan(g3, layers=[0, 1, 3]), GRAPH, "layer 1: variable 3 occurs twice")
    assert plan(g3, layers=[0, 2, 3])["layers"]["maxlayer"] == 2


def test_type_refusals_in_their_order():
    def resolve(algo, corr=0.75, max_iter=10, stream=0, g=SMALL, layers=(0, 8), **kw):
        return plan(g, 2, 6, 8, algo, corr, max_iter, stream, layers=layers, **kw)
    for algo in (5, -1, 5 | F32, 0x200):
        assert refused(resolve(algo), ARG, "unknown decoder type")
    # both flags: the "no binary32 form" message on every base type, before "layered min-sum only"
    for base in (SUMPROD2, L_SUMPROD2, L_MINSUM):
        assert refused(resolve(base | FIXED | F32), ARG, "LB_FIXED | LB_F32: the fixed-point decoder has no binary32 form")
    for base in (SUMPROD2, MINSUM, L_SUMPROD2):
        assert refused(resolve(base | FIXED), UNSUPPORTED, "fixed-point (LB_FIXED) exists for layered min-sum")
    assert refused(resolve(SUMPROD | F32), UNSUPPORTED, "binary32 (LB_F32) exists for the layered decoder types only")
    assert refused(resolve(MINSUM, stream=1), UNSUPPORTED, "the block stream exists for the layered decoder types only")
    assert refused(resolve(SUMPROD | F32, stream=1, max_iter=-1), UNSUPPORTED, "binary32 (LB_F32)")
    assert refused(resolve(L_MINSUM, max_iter=-1), ARG, "max_iter < 0")
    assert refused(resolve(L_MINSUM, max_iter=-1, layers=None), ARG, "max_iter < 0")
    assert refused(resolve(L_MINSUM, layers=None), ARG, "layered decoder on a context without layers (lb_set_layers)")
    assert refused(resolve(L_MINSUM | FIXED, layers=None), ARG, "layered decoder on a context without layers")
    for corr in (0.0, 0.03, 1.04, "nan"):  # rint(16 corr) = 0, 0, 17
        assert refused(resolve(L_MINSUM | FIXED, corr=corr), ARG, "fixed-point min-sum needs rint(16 corr_factor) in 1..16")
    # binary32 with app in HBM keeps it behind r in the word's message slice: the stream refuses up front
    wide = graph([2], [1, 1, 0])
    assert refused(resolve(L_SUMPROD2 | F32, stream=1, g=wide, layers=(0, 1), LAYERED_LDS=0), UNSUPPORTED,
                   "binary32 layered decoder without LDS needs Nv <= Nmsg")
    assert resolve(L_SUMPROD2 | F32, stream=0, g=wide, layers=(0, 1), LAYERED_LDS=0)["type"]["hbm"] == 1
    assert resolve(L_SUMPROD2 | F32, stream=1, g=wide, layers=(0, 1), LAYERED_LDS=1)["type"]["hbm"] == 1
    # what resolves
    t = resolve(L_MINSUM | FIXED, corr=0.7)["type"]
    assert (t["base"], t["f32"], t["fixed"], t["hbm"], t["par"]) == (L_MINSUM, 0, 1, 0, [2, 31, 127, 11])
    assert plan(SMALL, 3, 8, 16, L_MINSUM | FIXED, 1.0, 10, 1, layers=[0, 8])["type"]["par"] == [3, 127, 32767, 16]
    t = resolve(SUMPROD, max_iter=0, layers=None)["type"]
    assert (t["base"], t["f32"], t["fixed"], t["hbm"]) == (SUMPROD, 0, 0, 0)


@pytest.mark.parametrize("widths", [(-1, 6, 8), (9, 6, 8), (2, 1, 8), (2, 9, 9), (2, 6, 5), (2, 6, 17)])
def test_width_refusals(widths):
    assert refused(plan(SMALL, *widths), ARG, "fixed-point widths: frac_bits in 0..8, msg_bits in 2..8, app_bits in msg_bits..16")


def test_widths_at_their_limits():
    for widths in [(0, 2, 2), (8, 8, 16), (8, 8, 8)]:
        q = plan(SMALL, *widths)["fixed"]
        assert (q["qfrac"], q["qmsg"], q["qapp"], q["qnt"], q["qlanes"], q["qlds"], q["qfit"]) == widths + (0, 0, 0, 0)


# ---- the tail's grids ------------------------------------------------------------------------
# 802.16 1/2 z=24: Nc = 288 checks, 5 waves of 64 checks a word (9 of 32 on lane pairs); 256 CUs hold
# 1024 waves at one per SIMD; a workgroup has at most 2 waves (4 on lane pairs)

def tail(B, n, host, est_n, est_B, split):
    s = run("tail", B, n, host, est_n, est_B, 288, 256, split)
    return s["nsz"], s["cpt"], s["m"], s["S"]


def test_tail_shapes():
    assert tail(8, 3, 1, 0, 0, 0) == (3, 64, 1, 5)  # sized on the host: the words left, exactly
    assert tail(8, 3, 1, 50, 100, 0) == (3, 64, 1, 5)  # (an estimate is not looked at)
    assert tail(8, 8, 0, 0, 0, 0) == (8, 64, 1, 5)  # no estimate: a quarter with slack is 3, the floor 8
    assert tail(4, 4, 0, 0, 0, 0) == (4, 64, 1, 5)  # never more than the batch
    assert tail(1000, 1000, 0, 0, 0, 0) == (313, 64, 2, 3)  # ceil(0.25 * 1000 * 1.25); 1565 waves: m = 2
    assert math.ceil(10 / 100 * 1000 * 1.25) == 125
    assert tail(1000, 1000, 0, 10, 100, 0) == (125, 64, 1, 5)  # 625 waves
    assert tail(8, 3, 1, 0, 0, 1) == (3, 32, 1, 9)  # lane pairs: 32 checks a wave
    assert tail(1000, 1000, 0, 10, 100, 1) == (125, 32, 2, 5)  # 1125 waves: m = 2, ceil(288 / 64)
    assert tail(4000, 2000, 1, 0, 0, 0) == (2000, 64, 2, 3)  # 10000 waves: m = 10, capped at 2
    assert tail(4000, 2000, 1, 0, 0, 1) == (2000, 32, 4, 3)  # 18000 waves: capped at 4; ceil(288 / 128)


# ---- the graph tables ----------------------------------------------------------------------------

def fnv(values):
    h = 1469598103934665603
    for x in values:
        h = ((h ^ (int(x) & 0xffffffff)) * 1099511628211) & (2 ** 64 - 1)
    return h


@pytest.mark.parametrize("name", ["16_1/2_z3", "syn_dc8"])
def test_tables_against_numpy(name):
    if name == "syn_dc8":
        c = lc.make_code(name)
    else:
        from sparc_ldpc_amd import ldpc
        c = ldpc.code("802.16", "1/2", 3)
    vdeg, cdeg, intrlv = (np.asarray(a, dtype=np.int64) for a in (c.vdeg, c.cdeg, c.intrlv))
    p = plan((vdeg, cdeg, intrlv), "tables")
    t = {k: np.array(v["values"]) for k, v in p["tables"].items() if isinstance(v, dict)}
    Nv, maxdv = len(vdeg), int(vdeg.max())
    var_of_pos = np.repeat(np.arange(Nv), vdeg)  # the variable of port position p
    assert np.array_equal(t["evar"][intrlv], var_of_pos)
    first = np.concatenate([[0], np.cumsum(vdeg)])
    vedge = np.zeros((maxdv, Nv), dtype=np.int64)
    for j in range(Nv):
        vedge[:vdeg[j], j] = intrlv[first[j]:first[j + 1]]  # its k-th edge; 0 past its degree
    assert p["tables"]["maxdv_rows"] == maxdv and np.array_equal(t["vedge"], vedge.reshape(-1))
    assert np.array_equal(t["cstart"], np.concatenate([[0], np.cumsum(cdeg)]))
    assert np.array_equal(t["vdeg"], vdeg)
    for k, v in t.items():
        assert p["tables"][k]["size"] == len(v) and p["tables"][k]["fnv"] == fnv(v), k
    # without `tables`: the same checksums, no values
    brief = plan((vdeg, cdeg, intrlv))["tables"]
    assert all("values" not in brief[k] and brief[k]["fnv"] == p["tables"][k]["fnv"] for k in t)
