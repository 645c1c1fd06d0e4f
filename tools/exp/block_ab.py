#!/usr/bin/env python3
"""TAMD_FUSE_BLOCK off against on (block_i8.hip: an identity bottleneck block as one launch) on ONE box, one process:

  1. the device-resident step of the model in its default form (direct dispatch, the default split rule), the two graphs timed in
     turns (`rounds` alternations of `iters` steps), median of each; both pre-run from the SAME plan file, so every other launch of
     the two plans is the same kernel; outputs compared;
  2. per launch (tamd_graph_profile: hipEvent pairs, eager, one launch list of the whole batch): the launches of the fused blocks,
     three against one.

usage: block_ab.py [model=resnet50] [batch=32] [iters=300] [rounds=7]        (runs ON THE GPU BOX)"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tengine_amd import capi, models, tm2  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
batch = int(sys.argv[2]) if len(sys.argv) > 2 else 32
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 300
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
g = models.build(name, "int8", batch, device_only=True)
tmb = tm2.write_tm2(g)
x = models.synth_input(g, 3, tm2.DT_INT8)
os.environ.setdefault("TAMD_PLAN_CACHE", os.path.join(tempfile.gettempdir(), "block_ab_plan_%s_b%d_%d.txt" % (name, batch, os.getpid())))


def graph(fuse, **kw):
    os.environ["TAMD_FUSE_BLOCK"] = fuse
    try:
        gr = capi.Graph(tmb, batch=batch, **kw)
    finally:
        del os.environ["TAMD_FUSE_BLOCK"]
    gr.set_input(x)
    return gr


# ---- 1. the step ----
sides = [("off", graph("0", direct_dispatch=True)), ("on", graph("1", direct_dispatch=True))]
outs = {}
for nm, gr in sides:
    outs[nm] = [o.copy() for o in gr.run()]
    gr.upload()
    gr.sync()
    gr.time_launches(max(3, iters // 10))
same = all((a == b).all() for a, b in zip(outs["off"], outs["on"]))
res = {nm: [] for nm, _ in sides}
for r in range(rounds):
    for nm, gr in sides:
        res[nm].append(1e3 * gr.time_launches(iters) / iters)
print("== %s int8 b%d, device-resident step, us: %d alternations of %d steps, one process" % (name, batch, rounds, iters))
med = {}
for nm, gr in sides:
    v = sorted(res[nm])
    med[nm] = v[len(v) // 2]
    names = [k["kernel"] for k in gr.profile(1)]
    print("  TAMD_FUSE_BLOCK %-3s  min %8.2f  median %8.2f  max %8.2f | halves %d, launches %d (block_i8: %d), packets %d | every round: %s"
          % (nm, v[0], med[nm], v[-1], gr.halves(), gr.kernel_num(), names.count("block_i8"), gr.direct_packets(), " ".join("%.1f" % t for t in res[nm])))
    gr.close()
print("  on / off = %.4f (%+.1f us per step); outputs identical: %s" % (med["on"] / med["off"], med["on"] - med["off"], same))

# ---- 2. per launch ----
print("== per launch, one launch list of the whole batch (split_batch = 1), hipEvent pairs over 20 eager passes, us")
prof = {}
for nm, fuse in (("off", "0"), ("on", "1")):
    gr = graph(fuse, split_batch=1)
    gr.run()
    gr.profile(3)
    prof[nm] = gr.profile(20)
    gr.close()
blocks = [k["node"].split("+") for k in prof["on"] if k["kernel"] == "block_i8"]
for parts in blocks:
    three = [k for k in prof["off"] if k["node"] in parts]
    one = [k for k in prof["on"] if k["node"] == "+".join(parts)][0]
    for k in three:
        print("  off  %-28s %-40s %8.2f" % (k["node"], k["kernel"], 1e3 * k["ms"]))
    t3 = sum(1e3 * k["ms"] for k in three)
    print("  on   %-28s %-40s %8.2f   (three launches: %.2f; algorithmic MB %.1f, MMAC %.0f)"
          % (parts[0].rsplit("_", 1)[0], one["kernel"], 1e3 * one["ms"], t3, one["bytes"] / 1e6, one["macs"] / 1e6))
print("  sum of all launches: off %.1f us (%d launches), on %.1f us (%d launches)"
      % (sum(1e3 * k["ms"] for k in prof["off"]), len(prof["off"]), sum(1e3 * k["ms"] for k in prof["on"]), len(prof["on"])))
