#!/usr/bin/env python3
"""The directly dispatched pass -- the path bench.py's timed loop runs -- under the HSA runtime's own dispatch profiling
(tamd_graph_direct_timestamps: hsa_amd_profiling_get_dispatch_time per packet; csrc/direct.cc).  rocprofv3 cannot see this path (its
queue interceptor does not survive packets it did not see HIP write, so a traced process falls back to hipGraph replay); these are the
same start / end stamps a kernel trace reports, read without the tool.  Prints, per packet: kernel, mean duration, mean gap to the next
packet's start; and the sums against the step's own host clock.

usage: direct_timestamps.py <model> <batch> <int8|uint8> [passes]        (runs ON THE GPU BOX; TAMD_PLAN_CACHE honoured)"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tengine_amd import capi, models, plans, tm2  # noqa: E402


def short(sym):
    m = re.match(r"(?:void )?(?:tamd::)?([A-Za-z0-9_]+)(<[^(]*>)?", sym)
    return (m.group(1) + (m.group(2) or "")) if m else sym[:60]


def main():
    name, batch, dtype = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 200
    if "TAMD_PLAN_CACHE" not in os.environ:
        import tempfile
        p = os.path.join(tempfile.gettempdir(), "tamd_plan_ts_%d.txt" % os.getpid())
        plans.seed(p, name, dtype, batch)
        os.environ["TAMD_PLAN_CACHE"] = p
    g = models.build(name, dtype, batch)
    gr = capi.Graph(tm2.write_tm2(g), batch=batch, direct_dispatch=True)
    gr.set_input(models.synth_input(g, 1000, tm2.DT_UINT8 if dtype == "uint8" else tm2.DT_INT8))
    gr.upload()
    gr.sync()
    gr.time_launches(50)
    step_us = min(1e3 * gr.time_launches(passes) / passes for _ in range(3))
    rows = gr.direct_timestamps(passes)
    step_us2 = min(1e3 * gr.time_launches(passes) / passes for _ in range(3))
    halves = gr.halves()
    # a graph with two slots (tamd_options.split_batch, csrc/graph_slots.hip): the rows above are slot 0 ALONE, the chain as it is; then
    # ONE burst of alternating passes stamped on both queues (tamd_graph_slot_timestamps), raw stamps on the common clock
    two = None
    if gr.slots():
        import time

        def region():
            t0 = time.perf_counter()
            for _ in range(passes):
                gr.launch()
            gr.sync()
            return 1e6 * (time.perf_counter() - t0) / passes
        region()
        two = (min(region() for _ in range(3)),) + gr.slot_timestamps(min(passes, 60))
    gr.close()
    if halves:
        print("(the graph is two device graphs of batch %d side by side on their own queues, tamd_options.split_batch: the first half of the rows is the first "
              "half's launch list, stamped alone, then the second's -- the host clock is the two lists OVERLAPPED, so the sums below exceed it)" % (batch // 2))
    print("%s %s batch %d: %d packets per pass, %d passes back to back; host clock %.2f us per step before, %.2f after the stamped passes" % (name, dtype, batch, len(rows), passes, step_us, step_us2))
    print("%-4s %-58s %10s %14s" % ("#", "kernel", "us", "gap to next us"))
    for i, (sym, d, gp) in enumerate(rows):
        print("%-4d %-58s %10.2f %14.2f" % (i, short(sym)[:58], d, gp))
    sd, sg = sum(r[1] for r in rows), sum(r[2] for r in rows)
    print("sum of durations %.2f us + sum of gaps %.2f us = %.2f us per pass (device stamps; every packet carries a completion signal here, the timed loop's carry none)" % (sd, sg, sd + sg))
    print("mean duration %.2f us, mean gap %.2f us; host clock of the unstamped pass: %.2f us" % (sd / len(rows), sg / len(rows), step_us))
    if two:
        two_slots_report(rows, *two)


def two_slots_report(rows, thr_us, t0, t1):
    """t0 / t1[round, slot, packet]: one burst of alternating passes on the two queues.  How much of the burst do two packets run at once,
    and what does a packet cost overlapped against alone?"""
    import numpy as np
    if t0.shape[0] > 2:                 # the burst's first and last round run partly alone (ramp-up, drain): the middle is the steady state
        t0, t1 = t0[1:-1], t1[1:-1]
    lo, hi = float(t0.min()), float(t1.max())
    ev = sorted([(float(a), 1) for a in t0.reshape(-1)] + [(float(b), -1) for b in t1.reshape(-1)])
    busy = [0.0, 0.0, 0.0]
    depth, last = 0, lo
    for t, d in ev:
        busy[min(depth, 2)] += t - last
        depth, last = depth + d, t
    span = hi - lo
    n_pass = t0.shape[0] * 2
    print("-- two slots: %d rounds of (slot 0 pass, slot 1 pass) in one burst, both queues stamped; host clock of the unstamped loop %.2f us per pass" % (t0.shape[0], thr_us))
    print("share of the burst with two packets running %.1f %%, with one %.1f %%, with none %.1f %%; %.2f us of burst per pass (stamped)"
          % (100 * busy[2] / span, 100 * busy[1] / span, 100 * busy[0] / span, span / n_pass))
    print("%-4s %-58s %10s %12s %12s %9s" % ("#", "kernel", "alone us", "slot 0 us", "slot 1 us", "stretch"))
    d = (t1 - t0).mean(axis=0)           # [slot, packet]
    for i, (sym, alone, _) in enumerate(rows):
        print("%-4d %-58s %10.2f %12.2f %12.2f %8.2fx" % (i, short(sym)[:58], alone, d[0, i], d[1, i], d[:, i].mean() / alone if alone > 0 else 0.0))
    sa = sum(r[1] for r in rows)
    print("sum of packet durations per pass: alone %.2f us, overlapped slot 0 %.2f, slot 1 %.2f (stretch %.2fx); two passes at a time make %.2f us per pass of it"
          % (sa, d[0].sum(), d[1].sum(), d.sum() / (2 * sa), d.sum() / 4))


if __name__ == "__main__":
    main()
