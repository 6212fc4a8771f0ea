#!/usr/bin/env python3
"""Per-kernel durations inside the timed, graph-replayed region of a bench run
from a rocprofv3 --kernel-trace CSV (diagnostic).

The bench issues warmup + K graph replays, then eager profiling decodes; the
rocprofv3 --stats summary averages all of them.  This prints, per kernel, the
median / mean duration and the median gap to the next dispatch over the
dispatches of the graph-replayed decodes of the timed steps, plus the
per-decode wall time.

Two durations per kernel:
  * "duration": End - Start of the dispatch.  Inside a replayed graph the
    profiler's Start precedes the wait on the predecessor's completion, so
    these overlap: their sum over a decode exceeds the decode's wall time.
  * "exclusive": End - End of the preceding kernel of the decode (the first
    kernel: End - Start), i.e. the kernel plus the same-stream boundary in
    front of it; these add up to the decode's wall time exactly, and are what
    bench.py's back-to-back HIP-event timing measures.

Kernels are attributed to decodes per (queue, stream) of the trace: with decode
lanes two consecutive decodes run on two streams and interleave in one
timeline.  When the timed decodes sit on more than one stream the summary adds
how many of them overlap a decode of another stream, the overlapped share of
their wall time and the decode period (the in-graph durations then measure a
shared chip).

Since the fused tail a one-codeword decode with the
early stop off ends with its last section launch and no k_decide follows, so
on one stream consecutive decodes form one unbroken run of loop kernels (row,
section, row, ...).  The optional fourth argument gives the loop kernels of one
decode (2 T); longer runs are cut into decodes of that many.  The summary also
counts the k_decide dispatches of the whole trace.

Usage: graph_trace.py <kernel_trace.csv> [out.txt] [source-hash] [loop kernels per decode]
"""
import csv
import statistics as st
import sys

sys.path.insert(0, __file__.rsplit("/", 1)[0])
from pmc_summary import short  # noqa: E402

LOOP = ("k_sec4", "k_sec43", "k_sec44", "k_sec2", "k_sec", "k_secb", "k_row2", "k_rowv", "k_rowc", "k_row", "k_gemm_i8_Az", "k_gemm_i8_Ab", "k_gemm_f_Az", "k_gemm_f_Ab",
        "k_dense_az", "k_dense_ab", "k_dense_den", "k_i8_quant")


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    streams = {}
    for r in rows:
        key = (r.get("Queue_Id", ""), r.get("Stream_Id", ""))
        streams.setdefault(key, []).append(
            (short(r["Kernel_Name"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    # one decode = a maximal run of loop kernels: whatever else the stream
    # carries (the fills and k_iters_final / k_beta_final of the paths that
    # launch them, k_decide behind every step, conversions, copies) ends a run.
    # The graph replays are the decodes whose dispatches follow each other with
    # no host gap (median gap < 1 us), the eager profiling decodes have launch gaps
    runs, where = [], []
    for key, seq in streams.items():
        cur = []
        for k in seq + [("", 0, 0, "")]:
            if k[0] in LOOP:
                cur.append(k[:3])
            else:
                if cur:
                    runs.append(cur)
                    where.append(key)
                cur = []
    per_decode = int(sys.argv[4]) if len(sys.argv) > 4 else 0
    if per_decode:
        cut, cut_where = [], []
        for r, w in zip(runs, where):
            for i in range(0, len(r), per_decode):
                cut.append(r[i:i + per_decode])
                cut_where.append(w)
        runs, where = cut, cut_where

    def med_gap(r):
        return st.median([r[i + 1][1] - r[i][2] for i in range(len(r) - 1)]) if len(r) > 1 else 1e9
    timed = [(r, w) for r, w in zip(runs, where) if len(r) > 2 and med_gap(r) < 1000]
    if not timed:
        sys.exit("no graph-replayed decode found")
    n0 = st.mode([len(r) for r, _ in timed])
    timed = sorted([(r, w) for r, w in timed if len(r) == n0], key=lambda x: x[0][0][1])
    lanes = sorted({w for _, w in timed})
    timed, where = [r for r, _ in timed], [w for _, w in timed]
    out = []
    if len(sys.argv) > 3:
        out.append(f"sources sha256 {sys.argv[3]}")
    out.append(f"{len(timed)} graph-replayed decodes of {n0} loop kernels each")
    n_decide = sum(1 for seq in streams.values() for k in seq if k[0] == "k_decide")
    out.append(f"k_decide dispatches in the whole trace: {n_decide}")
    per = {}
    for r in timed:
        for i, (k, s, e) in enumerate(r):
            d = per.setdefault(k, {"dur": [], "gap": [], "exc": []})
            d["dur"].append(e - s)
            d["exc"].append(e - (r[i - 1][2] if i > 0 else s))
            if i + 1 < len(r):
                d["gap"].append(r[i + 1][1] - e)
    for k, d in per.items():
        out.append(f"{k:14s} n={len(d['dur']):5d}  duration median {st.median(d['dur']):8.0f} ns  mean "
                   f"{st.mean(d['dur']):8.0f} ns  min {min(d['dur']):7d}  gap to next median "
                   f"{st.median(d['gap']) if d['gap'] else 0:6.0f} ns  exclusive median {st.median(d['exc']):8.0f} ns"
                   f"  mean {st.mean(d['exc']):8.0f} ns")
    walls = [r[-1][2] - r[0][1] for r in timed]
    sums = [sum(e - s for _, s, e in r) for r in timed]
    out.append(f"replay wall (first start -> last end): median {st.median(walls) / 1e3:.1f} us; "
               f"sum of durations median {st.median(sums) / 1e3:.1f} us")
    if len(lanes) > 1:
        # two decodes of different streams in flight at once: the share of a
        # decode's wall time during which a decode of another stream runs, and
        # the period between the starts of consecutive decodes (any stream)
        share, hit = [], 0
        for i, r in enumerate(timed):
            a, b = r[0][1], r[-1][2]
            ov = 0
            for j in range(max(0, i - 3), min(len(timed), i + 4)):
                if j != i and where[j] != where[i]:
                    ov += max(0, min(b, timed[j][-1][2]) - max(a, timed[j][0][1]))
            hit += ov > 0
            share.append(min(1.0, ov / (b - a)))
        period = [timed[i + 1][0][1] - timed[i][0][1] for i in range(len(timed) - 1)]
        per_lane = ", ".join(f"queue {q} stream {s}: {where.count((q, s))}" for q, s in lanes)
        out.append(f"decodes on {len(lanes)} streams ({per_lane}); {hit} of {len(timed)} overlap a decode of another "
                   f"stream, overlapped share of a decode's wall time median {st.median(share):.2f}; "
                   f"decode period (start to next start, any stream) median {st.median(period) / 1e3:.1f} us")
    txt = "\n".join(out)
    print(txt)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(txt + "\n")


if __name__ == "__main__":
    main()
