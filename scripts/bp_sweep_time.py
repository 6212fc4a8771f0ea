"""Cost of one flooding iteration against one layered sweep (802.16 rate 5/6
z=192, sumprod2) on words that never converge (i.i.d. Gaussian LLRs), so that
every word runs exactly max_iter: device time of lb_run at max_iter = 4 and
12, the difference over 8 being the time of an iteration or sweep of a whole
launch of B words.  Flooding with the tail off (one workgroup per word, as the
layered kernel); the layered decoder as the library lays it out itself
("layered": r and app in LDS, 768 threads, the checks on the first 192, gather
and scatter over all) and with r held in HBM (LDPC_BP_LAYERED_LDS = 1), each
also at a thread per check (LDPC_BP_LAYERED_THREADS = 192).  Every layered
leg records its layout.  Prints one JSON line and writes it to
results/bp_sweep_time.json (or the second argument).

    python scripts/bp_sweep_time.py [B,B,... [out.json]]

--f32 (first argument): the binary32 layered decoders (LB_F32) against the
binary64 ones instead, sumprod2 and minsum: as the library lays them out (two
768-thread workgroups resident on a CU), held to one resident workgroup
(LDPC_BP_LAYERED_F32_RESIDENT = 1) and at 384 threads.  One context per leg,
a warm-up of each, then five rounds with the legs interleaved; written to
results/bp_sweep_time_f32.json.  The library is the one LDPC_BP_LIB names
(recorded as "library"): run it once more on a -DLB_F32_OCML build (make
f32_ocml) for the device library's expf / logf against the hardware's.

    python scripts/bp_sweep_time.py --f32 [B,B,... [out.json]]

--fixed (first argument): the fixed-point layered min-sum decoder (LB_FIXED,
widths 2, 6, 8) against binary64 and binary32 layered min-sum, corr_factor 0.75:
as the library plans it (lanes per check and threads per workgroup of its own
choice) and with the alternatives named by LDPC_BP_FIXED_LANES /
LDPC_BP_FIXED_THREADS.  The --f32 protocol; every fixed-point leg records
lb_fixed_info (threads, lanes, LDS bytes, resident workgroups).  Written to
results/bp_sweep_time_fixed.json.

    python scripts/bp_sweep_time.py --fixed [B,B,... [out.json]]
"""
import ctypes as ct
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparc_ldpc_amd import ldpc  # noqa: E402

D = ct.POINTER(ct.c_double)
lib = ldpc.load_bp_library()
assert lib.lb_device_count() > 0, "no HIP device visible"
F32 = len(sys.argv) > 1 and sys.argv[1] == "--f32"
FIXED = len(sys.argv) > 1 and sys.argv[1] == "--fixed"
if F32 or FIXED:
    del sys.argv[1]
BS = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [256, 1024]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
    ROOT, "results", "bp_sweep_time_f32.json" if F32 else "bp_sweep_time_fixed.json" if FIXED else "bp_sweep_time.json")


def f32_legs():
    env = ("LDPC_BP_LAYERED_F32_RESIDENT", "LDPC_BP_LAYERED_THREADS")
    legs = {}
    for a in ("sumprod2", "minsum"):
        legs[f"{a}_f64"] = (f"layered_{a}", None, None)
        legs[f"{a}_f32"] = (f"layered_{a}_f32", None, None)
        legs[f"{a}_f32_one_resident"] = (f"layered_{a}_f32", "1", None)
        legs[f"{a}_f32_384"] = (f"layered_{a}_f32", None, "384")
        legs[f"{a}_f64_384"] = (f"layered_{a}", None, "384")
    codes = {}
    for leg, (dectype, *knobs) in legs.items():
        for name, val in zip(env, knobs):
            os.environ.pop(name, None)
            if val is not None:
                os.environ[name] = val
        c = ldpc.code("802.16", "5/6", 192)
        c._algo(dectype)  # sets the layers under this leg's switches
        codes[leg] = c
    for name in env:
        os.environ.pop(name, None)
    out = {"library": os.path.basename(ldpc.LIB_PATH), "rounds": 5}
    for B in BS:
        CH = np.ascontiguousarray(3.0 * np.random.RandomState(B).randn(B, codes["sumprod2_f64"].N))
        for leg, c in codes.items():
            assert lib.lb_stage(c._context(), B, CH.ctypes.data_as(D)) == 0
            for k in (4, 12):
                c.run_buffers(B, legs[leg][0], max_iter=k)  # warm-up
        t = {leg: {4: [], 12: []} for leg in legs}
        for _ in range(5):
            for leg, c in codes.items():
                for k in (4, 12):
                    c.run_buffers(B, legs[leg][0], max_iter=k)
                    t[leg][k].append(c.mc_event_ms())
                    assert (c.fetch_buffers(B, app=False)[1] == k).all()  # no word stopped early
        for leg in legs:
            sweeps = [(b - a) / 8 * 1e3 for a, b in zip(t[leg][4], t[leg][12])]
            out.setdefault(leg, {})[str(B)] = dict(ms_at_4=t[leg][4], ms_at_12=t[leg][12], us_per_launch_sweep=sweeps,
                                                   median_us_per_launch_sweep=statistics.median(sweeps))
    for leg, c in codes.items():
        out[leg]["layout"] = c.layer_info("f32" if "_f32" in leg else "f64")
    return out


def fixed_legs():
    env = ("LDPC_BP_FIXED_LANES", "LDPC_BP_FIXED_THREADS")
    M, CORR, WIDTHS = "layered_minsum", 0.75, ldpc.FIXED_DEFAULT
    # leg -> (decoder, quant, LDPC_BP_FIXED_LANES, LDPC_BP_FIXED_THREADS), read when the leg's code sets its layers
    legs = {"minsum_f64": (M, None, None, None), "minsum_f32": (M + "_f32", None, None, None),
            "fixed": (M, WIDTHS, None, None)}
    for lanes, threads in ((1, None), (2, None), (8, None), (16, None), (2, "192"), (2, "768"), (4, "384"), (4, "768"),
                           (1, "384")):
        legs[f"fixed_lanes{lanes}" + (f"_threads{threads}" if threads else "")] = (M, WIDTHS, str(lanes), threads)
    codes = {}
    for leg, (dectype, quant, *knobs) in legs.items():
        for name, val in zip(env, knobs):
            os.environ.pop(name, None)
            if val is not None:
                os.environ[name] = val
        codes[leg] = ldpc.code("802.16", "5/6", 192)
    out = {"library": os.path.basename(ldpc.LIB_PATH), "rounds": 5, "corr_factor": CORR, "widths": list(WIDTHS)}
    for B in BS:
        CH = np.ascontiguousarray(3.0 * np.random.RandomState(B).randn(B, codes["fixed"].N))

        def run(leg, k):
            # the leg's switches stand while it runs: lb_set_layers and lb_set_fixed (every quant= call) read them
            for name, val in zip(env, legs[leg][2:]):
                os.environ.pop(name, None)
                if val is not None:
                    os.environ[name] = val
            c = codes[leg]
            c.run_buffers(B, legs[leg][0], CORR, k, quant=legs[leg][1])
            return c.mc_event_ms()

        for leg, c in codes.items():
            assert lib.lb_stage(c._context(), B, CH.ctypes.data_as(D)) == 0
            for k in (4, 12):
                run(leg, k)  # warm-up
        t = {leg: {4: [], 12: []} for leg in legs}
        for _ in range(5):
            for leg, c in codes.items():
                for k in (4, 12):
                    t[leg][k].append(run(leg, k))
                    assert (c.fetch_buffers(B, app=False)[1] == k).all()  # no word stopped early
        for leg in legs:
            sweeps = [(b - a) / 8 * 1e3 for a, b in zip(t[leg][4], t[leg][12])]
            out.setdefault(leg, {})[str(B)] = dict(ms_at_4=t[leg][4], ms_at_12=t[leg][12], us_per_launch_sweep=sweeps,
                                                   median_us_per_launch_sweep=statistics.median(sweeps))
        fx, f32 = out["fixed"][str(B)]["us_per_launch_sweep"], out["minsum_f32"][str(B)]["us_per_launch_sweep"]
        out.setdefault("bar_every_fixed_round_below_every_f32_round", {})[str(B)] = bool(max(fx) < min(f32))
        for leg, c in codes.items():  # (as the leg's last run planned it)
            out[leg]["layout"] = c.fixed_info() if legs[leg][1] else c.layer_info("f32" if "_f32" in leg else "f64")
            if legs[leg][1]:
                assert legs[leg][2] in (None, str(out[leg]["layout"]["lanes"])), (leg, out[leg]["layout"])
    for name in env:
        os.environ.pop(name, None)
    return out


if F32 or FIXED:
    out = fixed_legs() if FIXED else f32_legs()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    sys.exit(0)
L = "layered_sumprod2"
# leg -> (decoder, LDPC_BP_LAYERED_LDS, LDPC_BP_LAYERED_THREADS), read when the leg's code sets its layers
LEGS = {"flooding": ("sumprod2", None, None), "layered": (L, None, None), "layered_192": (L, None, "192"),
        "layered_r_hbm": (L, "1", None), "layered_r_hbm_192": (L, "1", "192")}
ENV = ("LDPC_BP_LAYERED_LDS", "LDPC_BP_LAYERED_THREADS")
out = {}
for leg, (dectype, *knobs) in LEGS.items():
    for name, val in zip(ENV, knobs):
        os.environ.pop(name, None)
        if val is not None:
            os.environ[name] = val
    c = ldpc.code("802.16", "5/6", 192)
    c.set_tail(0)
    for B in BS:
        CH = np.ascontiguousarray(3.0 * np.random.RandomState(B).randn(B, c.N))
        assert lib.lb_stage(c._context(), B, CH.ctypes.data_as(D)) == 0
        ms = {}
        for k in (4, 12):
            c.run_buffers(B, dectype, max_iter=k)  # warm-up
            t = []
            for _ in range(5):
                c.run_buffers(B, dectype, max_iter=k)
                t.append(c.mc_event_ms())
            assert (c.fetch_buffers(B, app=False)[1] == k).all()  # no word stopped early
            ms[k] = statistics.median(t)
        out.setdefault(leg, {})[str(B)] = dict(ms_at_4=ms[4], ms_at_12=ms[12],
                                               us_per_launch_iteration=(ms[12] - ms[4]) / 8 * 1e3)
    if dectype == L:
        out[leg]["layout"] = c.layer_info()
for name in ENV:
    os.environ.pop(name, None)
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(json.dumps(out, indent=1) + "\n")
