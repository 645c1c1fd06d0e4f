#!/usr/bin/env python3
"""The measurements behind profiles/crop_topdown.txt (runs ON THE GPU BOX, prints the tables):

  (a) RetinaFace's top-down merge between its convolutions (tests/crop_helpers.py: pyramid_graph, 64 channels, the MXNet-form Crop of
      retinaface_benchmark.tmfile) at the file's own map sizes for a 320 x 240 input -- lateral (1,64,15,20), small map (1,64,8,10), and the second merge, lateral (1,64,30,40), small map
      (1,64,15,20), where the Crop cuts nothing -- and
      for a 640 x 640 input -- (1,64,80,80) and (1,64,40,40) -- through the plugin: create_graph / prerun_graph / run_graph of the
      unmodified reference library on device "HIP".  Four sides, one child process per run, in alternation: the plugin of ANOTHER build
      (the parent commit: the directory given as argument holds its libtengine_hip_device.so and libtengine_amd.so), this tree's with
      TAMD_PIN=topdown=1 (topdown_u8), with TAMD_PIN=topdown=0 (Interp + Crop as one launch, eltwise_u8) and with TAMD_PIN=crop_chain=0
      (three launches).  Host to host run_graph time, median of RUNS runs after WARM warm-up runs; outputs compared with the CPU device
  (b) the launches themselves on the same graphs, one process, alternating rounds of tamd_graph_profile: topdown_u8 beside eltwise_u8,
      interp_nearest_u8 (with the Crop inside and without) and slice_u8 on the same output bytes

    python tools/crop_profile.py [directory of the other build's two libraries]
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

import crop_helpers as ch  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 200, 5
BLOCKS = {"320x240": lambda: ch.pyramid_graph(DT_UINT8, (1, 64, 15, 20), crop=ch.MXNET2),
          "320x240 (second merge)": lambda: ch.pyramid_graph(DT_UINT8, (1, 64, 30, 40), crop=ch.MXNET2), "640x640": lambda: ch.pyramid_graph(DT_UINT8, (1, 64, 80, 80), crop=ch.MXNET2)}


def child(plugin, case):
    """one process, one plugin: prints `subgraphs median_us equal`"""
    from oracle import ref_capi as ref
    import test_plugin_dropin as tp
    tp.PLUGIN = plugin
    tp._load_plugin(ref)
    g, x = BLOCKS[case]()
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
    print("  %-52s median %8.2f  min %8.2f  max %8.2f  spread %6.2f | %s" % (name, statistics.median(vals), min(vals), max(vals), max(vals) - min(vals),
                                                                           " ".join("%.2f" % v for v in vals)))


def blocks(other):
    mine = os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so")
    sides = [("this plugin, topdown=1: topdown_u8", mine, "topdown=1"), ("this plugin, topdown=0: chain + eltwise_u8", mine, "topdown=0"),
             ("this plugin, crop_chain=0: three launches", mine, "crop_chain=0")]
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
                if out.returncode != 0 or not r:          # a dead child may have faulted the GPU: nothing more is started on it
                    print("  %s %s: child exited with status %d; stopping here.  %s" % (case, side, out.returncode, out.stderr[-300:]))
                    return out.returncode or 1
                _, pl, us, eq = r[0].split()
                assert eq == "1", (case, side, "outputs differ from the CPU device")
                res[side].append(float(us))
                placed[side] = pl
        g, _ = BLOCKS[case]()
        print("pyramid block for a %s input, lateral %s" % (case, tuple(g.tensors[0].dims)))
        for side, _, _ in sides:
            line("%s: %s" % (side, placed[side]), res[side])
    return 0


def launches(rounds=9, iters=200):
    """every form of every block lives in this process, timed in alternation, one round of all of them thrown away first; per kernel
    name the sum over its launches, us per launch (tamd_graph_profile: eager, one event pair around `iters` back-to-back launches)"""
    ours = ("topdown_u8", "interp_nearest_u8", "slice_u8", "eltwise_u8")
    for case in BLOCKS:
        g, x = BLOCKS[case]()
        b = tm2.write_tm2(g)
        graphs = {}
        for name, pin in (("topdown=1", "topdown=1"), ("topdown=0", "topdown=0"), ("crop_chain=0", "crop_chain=0")):
            if pin:
                os.environ["TAMD_PIN"] = pin
            try:
                gr = capi.Graph(b)
            finally:
                os.environ.pop("TAMD_PIN", None)
            gr.set_input(x)
            graphs[name] = (gr, gr.run())
        res = {}
        for r in range(rounds + 1):
            for name, (gr, _) in graphs.items():
                prof = gr.profile(iters)
                if r == 0:
                    continue
                for k in ours:
                    hit = [p["ms"] * 1e3 for p in prof if p["kernel"] == k]
                    if hit:
                        res.setdefault((name, k), []).append(sum(hit))
                res.setdefault((name, "all four, their sum"), []).append(sum(p["ms"] * 1e3 for p in prof if p["kernel"] in ours))
        print("launches of the merge for a %s input, %d output bytes" % (case, int(np.prod(g.tensors[0].dims))))
        for (name, k), v in res.items():
            line("%s: %s" % (name, k), v)
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
    rc = blocks(sys.argv[1] if len(sys.argv) > 1 else None)
    if rc:
        sys.exit(rc)
    launches()
    sys.exit(0)
