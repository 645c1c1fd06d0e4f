#!/usr/bin/env python3
"""The measurements behind profiles/instnorm.txt (runs ON THE GPU BOX, prints the tables):

  (a) the generator block conv3x3 -> InstanceNorm -> ReLU -> conv3x3 through the plugin -- create_graph / prerun_graph / run_graph of the
      unmodified reference library on device "HIP" -- in uint8 at (1,32,128,128), (1,64,64,64) and (1,128,32,32)
      (tests/instnorm_helpers.py: generator_block).  Three sides, one child process per run, in alternation: the plugin of ANOTHER build
      (the parent commit: the directory given as argument holds its libtengine_hip_device.so and libtengine_amd.so), which leaves the
      node to the CPU device, and this tree's with TAMD_PIN=instnorm_form=0 and =1.  Host to host run_graph time, median of RUNS runs
      after WARM warm-up runs; outputs compared with the CPU device
  (b) the node's launches alone on data -> InstanceNorm -> ReLU graphs of those shapes and of (1,256,16,16) and (8,128,32,32), one
      process, alternating rounds of tamd_graph_profile: form 0 (instnorm_stats_u8 + chan_lut_u8, the apply step listed alone) beside
      form 1 (instnorm_u8), each with the ReLU folded and with TAMD_PIN=instnorm_relu=0 (a relu_u8 launch behind)
  (c) the chain: instnorm_stats_u8's time against H * W at plane counts that leave SIMDs idle -- the slope is the time of two dependent
      operations per element (one per pass), whatever N * C is

    python tools/instnorm_profile.py [directory of the other build's two libraries | -] [launches]
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

import instnorm_helpers as nh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 100, 3
BLOCKS = {"(1,32,128,128)": (1, 32, 128, 128), "(1,64,64,64)": (1, 64, 64, 64), "(1,128,32,32)": (1, 128, 32, 32)}
NODES = [(1, 32, 128, 128), (1, 64, 64, 64), (1, 128, 32, 32), (1, 256, 16, 16), (8, 128, 32, 32)]
OURS = ("instnorm_stats_u8", "chan_lut_u8", "instnorm_u8", "relu_u8")


def child(plugin, case):
    """one process, one plugin: prints `placement median_us equal`"""
    from oracle import ref_capi as ref
    import test_plugin_dropin as tp
    tp.PLUGIN = plugin
    tp._load_plugin(ref)
    d = BLOCKS[case]
    g, x = nh.generator_block(DT_UINT8, dims=d, cmid=d[1], cout=d[1])
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_UINT8)
    rg = ref.RefGraph(b, ref.MODE_UINT8, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
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
                                                                           " ".join("%.2f" % v for v in vals)))


def through_the_plugin(other):
    mine = os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so")
    sides = [("this plugin, instnorm_form=0", mine, "instnorm_form=0"), ("this plugin, instnorm_form=1", mine, "instnorm_form=1")]
    if other:
        sides.insert(0, ("parent plugin", os.path.join(other, "libtengine_hip_device.so"), None))
    for case in BLOCKS:
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
                if out.returncode != 0 or not r:      # a dead child may have faulted the GPU: nothing more is started on it
                    print("  %s %s: child exited with status %d; stopping here.  %s" % (case, side, out.returncode, out.stderr[-300:]))
                    return out.returncode or 1
                _, pl, us, eq = r[0].split()
                assert eq == "1", (case, side, "outputs differ from the CPU device")
                res[side].append(float(us))
                placed[side] = pl
        print("generator block on %s, uint8, us per run_graph" % case, flush=True)
        for side, _, _ in sides:
            line("%s: %s" % (side, placed[side]), res[side])
    return 0


def launches(nodes, rounds=7, iters=100):
    """the four variants of a node live in this process, timed in alternation, one round of all of them thrown away first; us per launch
    (tamd_graph_profile: eager, one event pair around `iters` back-to-back launches)"""
    chain = {}
    for dims in nodes:
        g, x = nh.relu_behind(dims)
        b = tm2.write_tm2(g)
        graphs, outs = {}, []
        for pin in ("instnorm_form=0", "instnorm_form=1", "instnorm_form=0,instnorm_relu=0", "instnorm_form=1,instnorm_relu=0"):
            os.environ["TAMD_PIN"] = pin
            try:
                gr = capi.Graph(b)
            finally:
                os.environ.pop("TAMD_PIN", None)
            gr.set_input(x)
            outs.append(gr.run()[0])
            graphs[pin] = gr
        assert all(np.array_equal(outs[0], o) for o in outs)
        res = {}
        for k in range(rounds + 1):
            for name, gr in graphs.items():
                prof = gr.profile(iters)
                if k == 0:
                    continue
                total = 0.0
                for pr in prof:
                    if pr["kernel"] in OURS:
                        res.setdefault((name, pr["kernel"]), []).append(pr["ms"] * 1e3)
                        total += pr["ms"] * 1e3
                res.setdefault((name, "all launches"), []).append(total)
        print("the launches alone: uint8 %s, %d planes of %d bytes" % (dims, dims[0] * dims[1], dims[2] * dims[3]), flush=True)
        for (name, k), v in res.items():
            line("%s: %s" % (name, k), v)
        chain[dims] = res[("instnorm_form=0", "instnorm_stats_u8")]
        for gr in graphs.values():
            gr.close()
    print("the chain: instnorm_stats_u8 against H * W (two passes of one dependent operation per element)")
    small = [d for d in nodes if d[0] * d[1] <= 256]
    base = min(small, key=lambda d: d[2] * d[3])
    for d in small:
        hw = d[2] * d[3]
        med = statistics.median(chain[d])
        slope = ""
        if d != base:
            ns = (med - statistics.median(chain[base])) * 1e3 / (2.0 * (hw - base[2] * base[3]))
            slope = "; against %s: %.2f ns per element and pass" % (base, ns)
        print("  %-18s %4d planes x %6d bytes: %8.2f us, %.2f ns per element and pass with the launch in it%s" % (d, d[0] * d[1], hw, med, med * 1e3 / (2.0 * hw), slope))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if capi.device_count() < 1:
        sys.exit("no GPU: nothing is measured")
    if not (len(sys.argv) > 2 and sys.argv[2] == "launches"):
        rc = through_the_plugin(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None)
        if rc:
            sys.exit(rc)
    launches(NODES)
    sys.exit(0)
