#!/usr/bin/env python3
"""The measurements behind profiles/bytemap_chains.txt (runs ON THE GPU BOX, prints the tables):

  (a) through the plugin -- create_graph / prerun_graph / run_graph of the unmodified reference library on device "HIP" -- the graphs
      of tests/bytemap_helpers.py at model sizes: conv -> SiLU -> conv at (1,64,80,80) and (1,256,20,20), the four-node HardSwish
      decomposition between two convolutions at (1,96,28,28), and the input normalisation SUB_SCALAR -> PROD_SCALAR in front of two
      convolutions at (1,3,112,112), int8 and uint8.  Three sides, one child process per run, in alternation: the plugin of ANOTHER
      build (the parent commit: the directory given as argument holds its libtengine_hip_device.so and libtengine_amd.so), this tree's
      (the chain as one lut_u8 launch) and this tree's with TAMD_PIN=bytemap_chain=0 (one launch per node).  Host to host run_graph
      time, median of RUNS runs after WARM warm-up runs; outputs compared with the CPU device; the placement is printed
      -- and MobileFaceNet's two ends as one uint8 graph (bytemap_helpers.mobilefacenet_ends_graph) at the file's 112 x 112
  (c) the uint8 BatchNorm's two forms as launches, each pinned with TAMD_PIN=bn_form, on [1,128], [32,128], (1,64,7,7), (1,64,14,14),
      (1,64,28,28) and (1,64,56,56), with lut_u8 on the same byte count (the two Clip guards of bytemap_helpers.bn_guarded_graph) as
      the floor: where the ranges separate is the plane-size threshold of plan_batchnorm_u8
  (b) the launches themselves on the same graphs, one process, alternating rounds of tamd_graph_profile: the chain's one lut_u8 beside
      the lut_u8 / eltwise_* launches it replaces

    python tools/bytemap_profile.py [directory of the other build's two libraries] [bn: the BatchNorm parts alone]
"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import bytemap_helpers as bh  # noqa: E402
import lut_helpers as lh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_INT8, DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 200, 4
BLOCKS = {}
for _dt in (DT_INT8, DT_UINT8):
    _t = bh.TAG[_dt]
    BLOCKS["silu %s (1,64,80,80)" % _t] = (_dt, lambda dt=_dt: bh.silu_graph(dt, (1, 64, 80, 80), mid=64))
    BLOCKS["silu %s (1,256,20,20)" % _t] = (_dt, lambda dt=_dt: bh.silu_graph(dt, (1, 256, 20, 20), mid=256))
    BLOCKS["hardswish decomposition %s (1,96,28,28)" % _t] = (_dt, lambda dt=_dt: bh.hardswish_graph(dt, (1, 96, 28, 28)))
    BLOCKS["normalise %s (1,3,112,112)" % _t] = (_dt, lambda dt=_dt: bh.normalise_graph(dt, (1, 3, 112, 112)))


BLOCKS["mobilefacenet ends u8 (1,3,112,112)"] = (DT_UINT8, lambda: bh.mobilefacenet_ends_graph(1, 112))
BN_SHAPES = [(1, 128), (32, 128), (1, 64, 7, 7), (1, 64, 14, 14), (1, 64, 28, 28), (1, 64, 56, 56)]


def bn_launches(rounds=9, iters=200):
    """both forms of every shape live in this process, timed in alternation, one round thrown away: us per launch"""
    for dims in BN_SHAPES:
        g, x, _ = bh.bn_guarded_graph(dims, 3)
        b = tm2.write_tm2(g)
        graphs = {}
        for form in (0, 1):
            os.environ["TAMD_PIN"] = "bn_form=%d" % form
            try:
                gr = capi.Graph(b)
            finally:
                os.environ.pop("TAMD_PIN", None)
            gr.set_input(x)
            graphs[form] = (gr, gr.run())
        res = {}
        for r in range(rounds + 1):
            for form, (gr, _) in graphs.items():
                prof = gr.profile(iters)
                if r == 0:
                    continue
                for p in prof:
                    if p["kernel"] in ("chan_lut_u8", "prelu_u8"):
                        res.setdefault(p["kernel"], []).append(p["ms"] * 1e3)
                if form == 0:
                    res.setdefault("lut_u8 (the floor)", []).append(sum(p["ms"] * 1e3 for p in prof if p["kernel"] == "lut_u8") / 2)
        plane = int(np.prod(dims[2:])) if len(dims) > 2 else 1
        print("BatchNorm on %s: %d bytes, planes of %d" % (dims, int(np.prod(dims)), plane))
        for name, v in res.items():
            line(name, v)
        assert all(np.array_equal(a, c) for a, c in zip(graphs[0][1], graphs[1][1]))
        for gr, _ in graphs.values():
            gr.close()


def child(plugin, case):
    """one process, one plugin: prints `placement median_us equal`"""
    from oracle import ref_capi as ref
    import test_plugin_dropin as tp
    tp.PLUGIN = plugin
    tp._load_plugin(ref)
    dtype, build = BLOCKS[case]
    g, x = build()
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, dtype)
    want = ref.run_model(b, x, mode)
    rg = ref.RefGraph(b, mode, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
    rg.set_input(x)
    for _ in range(WARM):
        rg.run()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        rg.run()
        ts.append((time.perf_counter() - t0) * 1e6)
    got = rg.outputs()
    pl = [dev for dev, _, r, _ in tp.placement(rg) if r]
    rg.close()
    print("RESULT %s %.2f %d" % ("/".join(pl), statistics.median(ts), int(all(np.array_equal(w, o) for w, o in zip(want, got)))))


def line(name, vals):
    print("  %-58s median %8.2f  min %8.2f  max %8.2f  spread %6.2f | %s" % (name, statistics.median(vals), min(vals), max(vals), max(vals) - min(vals),
                                                                           " ".join("%.2f" % v for v in vals)), flush=True)


def blocks(other, only=None):
    mine = os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so")
    sides = [("this plugin: the chain as one lut_u8", mine, None), ("this plugin, bytemap_chain=0: one launch per node", mine, "bytemap_chain=0")]
    if other:
        sides.insert(0, ("parent plugin", os.path.join(other, "libtengine_hip_device.so"), None))
    for case in BLOCKS:
        if only and only not in case:
            continue
        res = {s[0]: [] for s in sides}
        placed = {}
        for _ in range(ROUNDS):
            for side, plugin, pin in sides:
                env = dict(os.environ)
                env.pop("TAMD_PIN", None)
                if pin:
                    env["TAMD_PIN"] = pin
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", plugin, case], capture_output=True, text=True, timeout=300, env=env)
                r = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                if out.returncode != 0 or not r:          # a dead child may have faulted the GPU: nothing more is started on it
                    print("  %s %s: child exited with status %d; stopping here.  %s" % (case, side, out.returncode, out.stderr[-300:]))
                    return out.returncode or 1
                _, pl, us, eq = r[0].split()
                assert eq == "1", (case, side, "outputs differ from the CPU device")
                res[side].append(float(us))
                placed[side] = pl
        print("%s through the plugin, us per run_graph" % case)
        for side, _, _ in sides:
            line("%s: %s" % (side, placed[side]), res[side])
    return 0


def launches(rounds=9, iters=200):
    """both plans of every block live in this process, timed in alternation, one round of both thrown away first; the sum over the
    byte-map and same-shape Eltwise launches, us (tamd_graph_profile: eager, one event pair around `iters` back-to-back launches)"""
    ours = ("lut_u8", "eltwise_i8", "eltwise_u8", "eltwise_relu_i8")
    for case, (dtype, build) in BLOCKS.items():
        g, x = build()
        b = tm2.write_tm2(g)
        graphs = {}
        for name, pin in (("one lut_u8", None), ("bytemap_chain=0", "bytemap_chain=0")):
            if pin:
                os.environ["TAMD_PIN"] = pin
            try:
                gr = capi.Graph(b)
            finally:
                os.environ.pop("TAMD_PIN", None)
            gr.set_input(x)
            graphs[name] = (gr, gr.run())
        res, listed = {}, {}
        for r in range(rounds + 1):
            for name, (gr, _) in graphs.items():
                prof = gr.profile(iters)
                if r == 0:
                    continue
                hit = [p for p in prof if p["kernel"] in ours]
                listed[name] = " + ".join(p["kernel"] for p in hit)
                res.setdefault(name, []).append(sum(p["ms"] * 1e3 for p in hit))
        m, chain = bh.chain_start(g), None
        chain = capi.bytemap_chain(b, m)[0]
        print("launches of the chain of %s, %d bytes per tensor, %d nodes" % (case, int(np.prod(g.tensors[g.nodes[chain[0]].inputs[0]].dims)), len(chain)))
        for name, v in res.items():
            line("%s: %s" % (name, listed[name]), v)
        outs = [o for _, o in graphs.values()]
        assert all(np.array_equal(outs[0][0], o[0]) for o in outs)
        for gr, _ in graphs.values():
            gr.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if capi.device_count() < 1:
        sys.exit("no GPU: nothing is measured")
    bn_only = len(sys.argv) > 2 and sys.argv[2] == "bn"
    rc = blocks(sys.argv[1] if len(sys.argv) > 1 else None, "mobilefacenet" if bn_only else None)
    if rc:
        sys.exit(rc)
    if not bn_only:
        launches()
    bn_launches()
    sys.exit(0)
