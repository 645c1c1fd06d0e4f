#!/usr/bin/env python3
"""Two passes in flight at batch 1?  The ceiling, measured before anything is built: two graphs of the same tmfile, each one launch list
on its own HSA queue (direct_dispatch, split_batch = 1), one plan file, the same input uploaded to both.  Two regions, interleaved in one
process: (a) one graph, 2K launch() then sync(); (b) the two graphs launched alternately, K each, then both synced -- 2K passes either
way, so us per pass compares directly.  Two graphs hold two copies of the weights: a floor for what one handle with shared weights
could reach.   usage: two_graphs_b1.py [model [steps [rounds [regions]]]]     (defaults: mobilenet_v1 2000 7 3)"""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tengine_amd import capi, models, plans, tm2  # noqa: E402


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "mobilenet_v1"
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    regions = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    plan = os.path.join(tempfile.gettempdir(), "two_graphs_b1_%d.txt" % os.getpid())
    os.environ["TAMD_PLAN_CACHE"] = plan
    shipped = plans.seed(plan, model, "int8", 1)          # the plan bench.py's headline runs on, when one is shipped
    g = models.build(model, "int8", 1)
    b = tm2.write_tm2(g)
    x = models.synth_input(g, 1000, tm2.DT_INT8)
    grs = []
    for _ in range(2):
        gr = capi.Graph(b, batch=1, direct_dispatch=True, split_batch=1)
        gr.set_input(x); gr.upload(); gr.sync()
        grs.append(gr)
    if not all(gr.direct_packets() for gr in grs):
        raise SystemExit("two_graphs_b1.py: a graph is not dispatched directly; nothing to measure")

    def one():
        t0 = time.perf_counter()
        for _ in range(2 * steps):
            grs[0].launch()
        grs[0].sync()
        return (time.perf_counter() - t0) / (2 * steps)

    def two():
        t0 = time.perf_counter()
        for _ in range(steps):
            grs[0].launch()
            grs[1].launch()
        grs[0].sync()
        grs[1].sync()
        return (time.perf_counter() - t0) / (2 * steps)

    def host_only():
        """what the submitting thread alone costs per launch(): a burst short enough to fit the ring, timed before its sync"""
        n = 8
        t0 = time.perf_counter()
        for _ in range(n):
            grs[0].launch()
        t = (time.perf_counter() - t0) / n
        grs[0].sync()
        return t

    one(); two()
    res = {"one": [], "two": []}
    for r in range(rounds):
        a = min(one() for _ in range(regions))
        c = min(two() for _ in range(regions))
        res["one"].append(1e6 * a)
        res["two"].append(1e6 * c)
        print("  round %d   one graph %7.2f us per pass   two graphs alternately %7.2f us per pass" % (r, 1e6 * a, 1e6 * c), flush=True)
    host = 1e6 * min(host_only() for _ in range(20))
    outs = [gr.download()[0] for gr in grs]
    same = np.array_equal(outs[0], outs[1])
    print("== %s int8 batch 1, device-resident, us per pass; %d rounds interleaved, min of %d x %d per round; %d packets per pass; plan %s" % (
        model, rounds, regions, steps, grs[0].direct_packets(), shipped or "timed in this process"))
    stat = {}
    for k, label in (("one", "(a) one graph, 2K launches"), ("two", "(b) two graphs alternately, K each")):
        v = sorted(res[k])
        stat[k] = (v[0], v[len(v) // 2], v[-1])
        print("  %-38s min %7.2f  median %7.2f  max %7.2f  spread %5.2f" % (label, v[0], v[len(v) // 2], v[-1], v[-1] - v[0]))
    spread = max(stat["one"][2] - stat["one"][0], stat["two"][2] - stat["two"][0])
    gain = stat["one"][1] - stat["two"][1]
    print("  (b) below (a) by %.2f us per pass (%+.1f %% images/s); three times the larger spread = %.2f us: %s" % (
        gain, 100.0 * (stat["one"][1] / stat["two"][1] - 1.0), 3 * spread, "the rule is met" if gain > 3 * spread else "the rule is NOT met"))
    print("  host cost of one launch() alone (8 launches, before their sync): %.2f us; outputs of the two graphs %s" % (host, "identical" if same else "DIFFER"))
    for gr in grs:
        gr.close()
    if os.path.exists(plan):
        os.remove(plan)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
