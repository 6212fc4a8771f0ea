#!/usr/bin/env python3
"""sim_ldpc (host draws / encode / count, GPU decode) against ldpc_mc.sim_ldpc_mc
(native draws, everything else on the device) at 802.16 5/6 z=192,
sigma = sqrt(1 / (2 * 10**(5.33/20))): exactly 8192 blocks each (MIN_ERRORS out
of reach, MAX_BLOCKS = 8192), batch 1024.  One warm-up of each, then the two
alternate three times in one process; every wall time is taken around a device
synchronise.  Prints one JSON line and writes it to results/ldpc_mc.json
(or --out): medians, spread, blocks/s, and the new path's split.

--draws device: the same protocol for sim_ldpc_mc with host draws against
sim_ldpc_mc(draws="device") (the blocks drawn on the GPU from their seeds), five
alternating rounds after a warm-up of each, written to
results/ldpc_mc_draws.json.  The bar: every device-draw run below every
host-draw run.

--dectype layered_sumprod2: sim_ldpc_mc(draws="device") with the flooding
sumprod2 against the layered decoder on the same seeds, as the library lays it
out itself (leg "layered": r and app in LDS, a thread per edge of a layer),
with r held in HBM (LDPC_BP_LAYERED_LDS = 1), and both at a thread per check
(LDPC_BP_LAYERED_THREADS = 192; "layouts" records each leg's), five
alternating rounds after a warm-up of each, written to
results/ldpc_mc_layered.json: per leg the median end-to-end and device
milliseconds, blocks/s, mean iterations or sweeps a block, bit and block
errors.  The flooding leg of the same session is the yardstick.

--dectype layered_sumprod2_f32 (or layered_minsum_f32), with --draws device:
the binary32 layered decoder against the binary64 layered one and the flooding
default on the same seeds, five alternating rounds after a warm-up of each,
written to results/ldpc_mc_f32.json: per leg and round end-to-end and device
milliseconds, sweeps a block, block and bit errors.  The bar of an opt-in
path: every binary32 round's device time below every binary64 layered
round's.  --sigma S runs the same legs at another noise level (fidelity: one
at which the binary64 decoder leaves block errors in every round); those
results are merged into the file under "fidelity", by sigma.

--stream: one operating point as a stream of refilled decoder slots
(code.mc_stream_seeds) against the batch path (code.mc_blocks_seeds) on the same
8192 seeds, draws on the device, layered_sumprod2_f32 and layered_sumprod2, at
sigma 0.5203 and 0.535, no stopping rule.  Legs: the batch path at batch 1024
and at batch 8192, the stream at chunk 1024 / 2048 / 4096 / 8192 with the
default slots, and at the default chunk with half and twice the slots.  After
a warm-up of each leg five interleaved rounds; per round end-to-end and device
milliseconds; every leg's per-block results are asserted equal to the batch
path's.  The bar of an opt-in path: at sigma 0.535 every round of the default
stream below every round of batch 1024, in device time, for both decoders.
Then the rule: sim_ldpc_mc(MIN_ERRORS=100) at both sigmas, at 0.48 (no block
fails) and at 0.56 (the rule is met within the first chunk) through batch
1024, batch 8192 and the stream, the dicts asserted equal, with the blocks
decoded against the blocks used.  Written to
results/ldpc_mc_stream.json.

--quant F,MB,AB (with --dectype layered_minsum and --draws device): the
fixed-point layered min-sum decoder (code.mc_blocks_seeds(quant=...)) against
layered_minsum_f32 on the same 8192 seeds at sigma 0.5203 and 0.535, batch 1024,
and with --stream also both through code.mc_stream_seeds at the default chunk;
five interleaved rounds after a warm-up of each leg, per round end-to-end and
device milliseconds.  The bar of an opt-in path: every fixed-point round below
every binary32 round of the same form, in device time.  Then fidelity (reported,
not gated): block and bit errors over the same seeds at sigma 0.5203, 0.535 and
0.56 for the widths given, (1, 4, 6) and (3, 8, 16), beside binary32 and
binary64 layered min-sum at the same corr_factor.  Written to
results/ldpc_mc_fixed.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS, BATCH, REPS = 8192, 1024, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--draws", default=None, choices=["device"],
                    help="time sim_ldpc_mc's host draws against its device draws instead")
    ap.add_argument("--dectype", default=None,
                    choices=["layered_sumprod2", "layered_minsum", "layered_sumprod2_f32", "layered_minsum_f32"],
                    help="time the flooding decoder against this layered one instead (device draws); _f32: "
                         "the binary32 layered decoder against the binary64 one and flooding")
    ap.add_argument("--sigma", type=float, default=None, help="noise level of the _f32 legs' fidelity run")
    ap.add_argument("--stream", action="store_true",
                    help="time the streamed operating point against the batch path instead")
    ap.add_argument("--quant", default=None, metavar="F,MB,AB",
                    help="with --dectype layered_minsum: time the fixed-point decoder of these widths against "
                         "layered_minsum_f32 (batch 1024; with --stream also streamed)")
    args = ap.parse_args()
    if args.quant:
        if args.dectype != "layered_minsum":
            ap.error("--quant goes with --dectype layered_minsum")
        return fixed_leg(args)
    if args.stream:
        return stream_leg(args)
    f32 = bool(args.dectype and args.dectype.endswith("_f32"))
    if args.out is None:
        name = "ldpc_mc_f32.json" if f32 else \
            "ldpc_mc_layered.json" if args.dectype else "ldpc_mc_draws.json" if args.draws else "ldpc_mc.json"
        args.out = os.path.join(ROOT, "results", name)
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible"
    lp = sp.LDPCParams("802.16", "5/6", 192)
    sigma = float(np.sqrt(1 / (2 * 10 ** (5.33 / 20))))
    never = 10 ** 9

    def sync():
        assert lib.hipDeviceSynchronize() == 0

    def old(seed):
        sync()
        t0 = time.perf_counter()
        ber = sp.sim_ldpc(lp, sigma, MIN_ERRORS=never, MAX_BLOCKS=BLOCKS, batch=BATCH, seed=seed)
        sync()
        return time.perf_counter() - t0, ber

    def new(seed0, draws="host", dectype=None, sigma=sigma):
        tm = {}
        kw = {} if draws == "host" else {"draws": draws}
        if dectype:
            kw["dectype"] = dectype
        sync()
        t0 = time.perf_counter()
        r = sp.sim_ldpc_mc(lp, sigma, MIN_ERRORS=never, MAX_BLOCKS=BLOCKS, seed0=seed0, batch=BATCH, timings=tm, **kw)
        sync()
        wall = time.perf_counter() - t0
        assert r["blocks"] == BLOCKS
        return wall, r, tm

    if f32:
        return f32_leg(args, new, sigma)
    if args.dectype:
        return layered_leg(args, new, sigma, lp)
    if args.draws:
        return draws_leg(args, new, sigma)
    old(1)
    new(1)
    t_old, t_new, bers_old, res_new, splits = [], [], [], [], []
    for k in range(REPS):
        w, ber = old(100 + k)
        t_old.append(w)
        bers_old.append(ber)
        w, r, tm = new(100_000 * (k + 1))
        t_new.append(w)
        res_new.append(r)
        splits.append(dict(wall_s=w, draw_s=tm["draw_s"], device_ms=tm["device_ms"],
                           rest_s=w - tm["device_ms"] / 1e3))
    med_old, med_new = statistics.median(t_old), statistics.median(t_new)
    spread = max(max(t_old) - min(t_old), max(t_new) - min(t_new))
    out = dict(
        workload="802.16 5/6 z=192, sigma=%.6f, %d blocks, batch %d" % (sigma, BLOCKS, BATCH),
        sim_ldpc=dict(wall_s=t_old, median_s=med_old, blocks_per_s=BLOCKS / med_old, ber=bers_old),
        sim_ldpc_mc=dict(wall_s=t_new, median_s=med_new, blocks_per_s=BLOCKS / med_new,
                         ber=[r["ber"] for r in res_new], block_errors=[r["block_errors"] for r in res_new],
                         nit_total=[r["nit_total"] for r in res_new], split=splits,
                         split_note="draw_s: native draws, in a worker thread beside the device work after the "
                                    "first round; device_ms: events around encode + BP + count; rest_s: wall "
                                    "minus device time (exposed draw, staging copies, Python)"),
        spread_s=spread, speedup=med_old / med_new,
        within_bar=bool(med_new <= med_old + spread),
    )
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


def draws_leg(args, new, sigma):
    rounds = 5
    new(1, "host")
    new(1, "device")
    runs = {"host": [], "device": []}
    for k in range(rounds):
        for draws in ("host", "device"):
            w, r, tm = new(100_000 * (k + 1), draws)
            runs[draws].append(dict(wall_s=w, draw_s=tm["draw_s"], device_ms=tm["device_ms"],
                                    rest_s=w - tm["device_ms"] / 1e3, ber=r["ber"], block_errors=r["block_errors"],
                                    nit_total=r["nit_total"]))
    med = {d: statistics.median(x["wall_s"] for x in runs[d]) for d in runs}
    out = dict(
        workload="802.16 5/6 z=192, sigma=%.6f, %d blocks, batch %d" % (sigma, BLOCKS, BATCH),
        host_draws=dict(runs=runs["host"], median_s=med["host"], blocks_per_s=BLOCKS / med["host"]),
        device_draws=dict(runs=runs["device"], median_s=med["device"], blocks_per_s=BLOCKS / med["device"]),
        split_note="device_ms: events around the whole run (host draws: encode + BP + count; device draws: the "
                   "draw kernels too); draw_s: the host draws' wall time, in a worker thread (0 for device draws); "
                   "rest_s: wall minus device time",
        speedup=med["host"] / med["device"],
        bar_every_device_run_below_every_host_run=bool(
            max(x["wall_s"] for x in runs["device"]) < min(x["wall_s"] for x in runs["host"])),
    )
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


def f32_leg(args, new, sigma0):
    rounds = 5
    sigma = args.sigma if args.sigma is not None else sigma0
    base = args.dectype[:-len("_f32")]
    legs = {"flooding": base[len("layered_"):], "layered_f64": base, "layered_f32": args.dectype}
    for dectype in legs.values():
        new(1, "device", dectype, sigma)
    runs = {leg: [] for leg in legs}
    for k in range(rounds):
        for leg, dectype in legs.items():
            w, r, tm = new(100_000 * (k + 1), "device", dectype, sigma)
            runs[leg].append(dict(wall_ms=w * 1e3, device_ms=tm["device_ms"], sweeps_per_block=r["nit_total"] / BLOCKS,
                                  block_errors=r["block_errors"], bit_errors=r["bit_errors"]))
    out = dict(workload="802.16 5/6 z=192, sigma=%.6f, %d blocks, batch %d, draws on the device, %s" %
               (sigma, BLOCKS, BATCH, args.dectype), rounds=rounds)
    for leg in legs:
        out[leg] = dict(median_wall_ms=statistics.median(x["wall_ms"] for x in runs[leg]),
                        median_device_ms=statistics.median(x["device_ms"] for x in runs[leg]), runs=runs[leg])
    out["speedup_device_f32_over_f64"] = out["layered_f64"]["median_device_ms"] / out["layered_f32"]["median_device_ms"]
    out["bar_every_f32_device_time_below_every_f64"] = bool(
        max(x["device_ms"] for x in runs["layered_f32"]) < min(x["device_ms"] for x in runs["layered_f64"]))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.sigma is not None and os.path.exists(args.out):  # the fidelity run joins the timing run's file
        with open(args.out) as fh:
            whole = json.load(fh)
        whole.setdefault("fidelity", {})["sigma_%g" % sigma] = out
        out = whole
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


def stream_leg(args):
    import sparc_ldpc_amd as sp
    from sparc_ldpc_amd import ldpc
    out_path = args.out or os.path.join(ROOT, "results", "ldpc_mc_stream.json")
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible"
    rounds, seeds = 5, np.arange(100_000, 100_000 + BLOCKS)
    lp = sp.LDPCParams("802.16", "5/6", 192)
    code = ldpc.code(lp.standard, lp.r_ldpc, lp.z, lp.ptype)
    default = ldpc.STREAM_CHUNK

    def timed(fn):
        assert lib.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        r = fn()
        assert lib.hipDeviceSynchronize() == 0
        return (time.perf_counter() - t0) * 1e3, code.mc_event_ms(), r

    out = dict(workload="802.16 5/6 z=192, %d blocks, draws on the device, no stopping rule" % BLOCKS, rounds=rounds,
               default_chunk=default, points={})
    for dectype in ("layered_sumprod2_f32", "layered_sumprod2"):
        full =code.mc_stream_seeds(seeds, 0.5, "awgn", BLOCKS, dectype)[2]["slots"]
        for sigma in (0.5203, 0.535):
            legs = {"batch_1024": lambda: code.mc_blocks_seeds(seeds, sigma, "awgn", 1024, dectype),
                    "batch_8192": lambda: code.mc_blocks_seeds(seeds, sigma, "awgn", 8192, dectype)}
            for chunk in (1024, 2048, 4096, 8192):
                legs["stream_%d" % chunk] = lambda chunk=chunk: code.mc_stream_seeds(seeds, sigma, "awgn", chunk, dectype)
            for name, n in (("half", full // 2), ("twice", full * 2)):
                legs["stream_%d_slots_%s" % (default, name)] = \
                    lambda n=n: code.mc_stream_seeds(seeds, sigma, "awgn", default, dectype, slots=n)
            ref = None
            for leg, fn in legs.items():  # warm-up, and every leg against the batch path
                r = fn()
                ref = ref or r
                assert np.array_equal(r[0], ref[0]) and np.array_equal(r[1], ref[1]), leg
            runs = {leg: [] for leg in legs}
            for _ in range(rounds):
                for leg, fn in legs.items():
                    wall, dev, _r = timed(fn)
                    runs[leg].append(dict(wall_ms=wall, device_ms=dev))
            pt = dict(default_slots=full, sweeps_per_block=float(ref[1].mean()), block_errors=int((ref[0] > 0).sum()))
            for leg in legs:
                pt[leg] = dict(median_device_ms=statistics.median(x["device_ms"] for x in runs[leg]),
                               median_wall_ms=statistics.median(x["wall_ms"] for x in runs[leg]), runs=runs[leg])
            dflt, a = runs["stream_%d" % default], runs["batch_1024"]
            pt["bar_every_stream_device_time_below_every_batch_1024"] = bool(
                max(x["device_ms"] for x in dflt) < min(x["device_ms"] for x in a))
            pt["speedup_device_over_batch_1024"] = pt["batch_1024"]["median_device_ms"] / \
                pt["stream_%d" % default]["median_device_ms"]
            pt["speedup_device_over_batch_8192"] = pt["batch_8192"]["median_device_ms"] / \
                pt["stream_%d" % default]["median_device_ms"]
            out["points"]["%s sigma=%g" % (dectype, sigma)] = pt
            print(dectype, sigma, {leg: round(pt[leg]["median_device_ms"], 3) for leg in legs}, flush=True)
    # the stopping rule
    out["rule"] = {}
    for dectype in ("layered_sumprod2_f32", "layered_sumprod2"):
        for sigma in (0.48, 0.5203, 0.535, 0.56):
            row = {}
            want = None
            for leg, kw in (("batch_1024", dict(batch=1024)), ("batch_8192", dict(batch=8192)),
                            ("stream", dict(batch=default, stream=True))):
                res = []
                for _ in range(3):
                    tm = {}
                    wall, _dev, r = timed(lambda: sp.sim_ldpc_mc(lp, sigma, MIN_ERRORS=100, MAX_BLOCKS=BLOCKS,
                                                                  seed0=100_000, draws="device", dectype=dectype,
                                                                  timings=tm, **kw))
                    want = want or r
                    assert r == want, (leg, r, want)
                    used = r["blocks"]
                    decoded = tm["stream"]["decoded"] if leg == "stream" else -(-used // kw["batch"]) * kw["batch"]
                    res.append(dict(wall_ms=wall, device_ms=tm["device_ms"], blocks_decoded=min(decoded, BLOCKS)))
                row[leg] = dict(median_wall_ms=statistics.median(x["wall_ms"] for x in res),
                                median_device_ms=statistics.median(x["device_ms"] for x in res), runs=res[1:],
                                first_run=res[0])
            row["result"] = want
            out["rule"]["%s sigma=%g" % (dectype, sigma)] = row
            print(dectype, sigma, "rule", want["blocks"],
                  {leg: (round(row[leg]["median_device_ms"], 3), row[leg]["runs"][-1]["blocks_decoded"])
                   for leg in ("batch_1024", "batch_8192", "stream")}, flush=True)
    out["bar_met"] = all(pt["bar_every_stream_device_time_below_every_batch_1024"]
                         for name, pt in out["points"].items() if name.endswith("0.535"))
    print(json.dumps({k: v for k, v in out.items() if k not in ("points", "rule")}))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


def fixed_leg(args):
    from sparc_ldpc_amd import ldpc
    out_path = args.out or os.path.join(ROOT, "results", "ldpc_mc_fixed.json")
    lib = ldpc.load_bp_library()
    assert lib.lb_device_count() > 0, "no HIP device visible"
    widths = tuple(int(x) for x in args.quant.split(","))
    rounds, seeds, corr = 5, np.arange(100_000, 100_000 + BLOCKS), 0.7
    code = ldpc.code("802.16", "5/6", 192)
    F32, M = "layered_minsum_f32", "layered_minsum"

    def timed(fn):
        assert lib.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        r = fn()
        assert lib.hipDeviceSynchronize() == 0
        return (time.perf_counter() - t0) * 1e3, code.mc_event_ms(), r

    out = dict(workload="802.16 5/6 z=192, %d blocks, draws on the device, corr_factor %g, widths %s" %
               (BLOCKS, corr, list(widths)), rounds=rounds, points={}, fidelity={})
    for sigma in (0.5203, 0.535):
        legs = {"f32_batch_1024": lambda: code.mc_blocks_seeds(seeds, sigma, "awgn", BATCH, F32, corr),
                "fixed_batch_1024": lambda: code.mc_blocks_seeds(seeds, sigma, "awgn", BATCH, M, corr, quant=widths)}
        if args.stream:
            legs["f32_stream"] = lambda: code.mc_stream_seeds(seeds, sigma, "awgn", ldpc.STREAM_CHUNK, F32, corr)[:2]
            legs["fixed_stream"] = lambda: code.mc_stream_seeds(seeds, sigma, "awgn", ldpc.STREAM_CHUNK, M, corr,
                                                                quant=widths)[:2]
        ref = {}
        for leg, fn in legs.items():  # warm-up; the streamed results are the batch path's
            r = fn()
            kind = leg.split("_")[0]
            ref.setdefault(kind, r)
            assert np.array_equal(r[0], ref[kind][0]) and np.array_equal(r[1], ref[kind][1]), leg
        runs = {leg: [] for leg in legs}
        for _ in range(rounds):
            for leg, fn in legs.items():
                wall, dev, _r = timed(fn)
                runs[leg].append(dict(wall_ms=wall, device_ms=dev))
        pt = {}
        for kind in ("f32", "fixed"):
            pt[kind + "_sweeps_per_block"] = float(ref[kind][1].mean())
            pt[kind + "_block_errors"] = int((ref[kind][0] > 0).sum())
        for leg in legs:
            pt[leg] = dict(median_device_ms=statistics.median(x["device_ms"] for x in runs[leg]),
                           median_wall_ms=statistics.median(x["wall_ms"] for x in runs[leg]), runs=runs[leg])
        for form in ("batch_1024",) + (("stream",) if args.stream else ()):
            a, b = runs["fixed_" + form], runs["f32_" + form]
            pt["bar_every_fixed_device_time_below_every_f32_" + form] = bool(
                max(x["device_ms"] for x in a) < min(x["device_ms"] for x in b))
            pt["speedup_device_over_f32_" + form] = pt["f32_" + form]["median_device_ms"] / \
                pt["fixed_" + form]["median_device_ms"]
        out["points"]["sigma=%g" % sigma] = pt
        print(sigma, {leg: round(pt[leg]["median_device_ms"], 3) for leg in legs}, flush=True)
    if args.stream:
        out["fixed_info"] = code.fixed_info()
        out["stream_slots"] = {"fixed": code.mc_stream_seeds(seeds[:1024], 0.5, quant=widths, dectype=M)[2]["slots"],
                               "f32": code.mc_stream_seeds(seeds[:1024], 0.5, dectype=F32)[2]["slots"]}
    # fidelity: the same seeds through every arithmetic (deterministic: a round repeats its counts)
    decoders = {"binary64": (M, None), "binary32": (F32, None)}
    for w in dict.fromkeys((widths, (1, 4, 6), (3, 8, 16))):
        decoders["fixed_%d_%d_%d" % w] = (M, w)
    for sigma in (0.5203, 0.535, 0.56):
        row = {}
        for name, (dectype, quant) in decoders.items():
            be, it = code.mc_blocks_seeds(seeds, sigma, "awgn", BATCH, dectype, corr, quant=quant)
            row[name] = dict(block_errors=int((be > 0).sum()), bit_errors=int(be.sum()), sweeps_per_block=float(it.mean()))
        out["fidelity"]["sigma=%g" % sigma] = row
        print(sigma, "fidelity", {k: (v["block_errors"], v["bit_errors"]) for k, v in row.items()}, flush=True)
    print(json.dumps({k: v for k, v in out.items() if k != "points"}))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


def layered_leg(args, new, sigma, lp):
    from sparc_ldpc_amd import ldpc
    rounds = 5
    flooding = args.dectype[len("layered_"):]
    # leg -> (dectype, LDPC_BP_LAYERED_LDS, LDPC_BP_LAYERED_THREADS read when the run's code sets its layers)
    legs = {"flooding": (flooding, None, None), "layered": (args.dectype, None, None),
            "layered_192": (args.dectype, None, "192"), "layered_r_hbm": (args.dectype, "1", None),
            "layered_r_hbm_192": (args.dectype, "1", "192")}
    names = ("LDPC_BP_LAYERED_LDS", "LDPC_BP_LAYERED_THREADS")

    def setenv(knobs):
        for name, val in zip(names, knobs):
            os.environ.pop(name, None)
            if val is not None:
                os.environ[name] = val

    def run(leg, seed0):
        dectype, *knobs = legs[leg]
        setenv(knobs)
        try:
            return new(seed0, "device", dectype)
        finally:
            setenv((None, None))

    layout = {}
    for leg, (dectype, *knobs) in legs.items():
        if leg == "flooding":
            continue
        setenv(knobs)
        c = ldpc.code(lp.standard, lp.r_ldpc, lp.z, lp.ptype)
        c.decode_batch(np.ones((1, c.N)), dectype, max_iter=1)
        layout[leg] = c.layer_info()
        setenv((None, None))
    for leg in legs:
        run(leg, 1)
    runs = {leg: [] for leg in legs}
    for k in range(rounds):
        for leg in legs:
            w, r, tm = run(leg, 100_000 * (k + 1))
            runs[leg].append(dict(wall_ms=w * 1e3, device_ms=tm["device_ms"], bit_errors=r["bit_errors"],
                                  block_errors=r["block_errors"], nit_total=r["nit_total"]))
    out = dict(workload="802.16 5/6 z=192, sigma=%.6f, %d blocks, batch %d, draws on the device, %s" %
               (sigma, BLOCKS, BATCH, args.dectype), rounds=rounds, layouts=layout)
    for leg in legs:
        wall = statistics.median(x["wall_ms"] for x in runs[leg])
        dev = statistics.median(x["device_ms"] for x in runs[leg])
        nit = statistics.mean(x["nit_total"] for x in runs[leg]) / BLOCKS
        out[leg] = dict(median_wall_ms=wall, median_device_ms=dev, blocks_per_s=BLOCKS / (wall / 1e3),
                        mean_iterations_or_sweeps=nit, device_us_per_block_iteration=dev * 1e3 / (BLOCKS * nit),
                        bit_errors=[x["bit_errors"] for x in runs[leg]],
                        block_errors=[x["block_errors"] for x in runs[leg]],
                        wall_ms=[x["wall_ms"] for x in runs[leg]], device_ms=[x["device_ms"] for x in runs[leg]])
    for leg in legs:
        if leg == "flooding":
            continue
        out[leg]["speedup_wall"] = out["flooding"]["median_wall_ms"] / out[leg]["median_wall_ms"]
        out[leg]["speedup_device"] = out["flooding"]["median_device_ms"] / out[leg]["median_device_ms"]
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
