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
BS = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [256, 1024]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "results", "bp_sweep_time.json")
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
