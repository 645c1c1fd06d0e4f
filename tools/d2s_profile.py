#!/usr/bin/env python3
"""The measurements behind profiles/d2s.txt (runs ON THE GPU BOX, prints the tables):

  (a) sub-pixel convolution through the plugin -- create_graph / prerun_graph / run_graph of the unmodified reference library on device
      "HIP" -- in int8 and uint8: the EDSR up-sampler conv -> DepthToSpace r 2 -> conv with the shuffle (1,64,64,64) -> (1,16,128,128),
      and the ESPCN tail conv -> ReLU -> conv -> DepthToSpace r 3 on (1,27,120,120) (tests/d2s_helpers.py).  Two sides, one child process
      per run, in alternation: the plugin of ANOTHER build (the parent commit: the directory given as argument holds its
      libtengine_hip_device.so and libtengine_amd.so), which leaves the node to the CPU device, and this tree's.  Host to host run_graph
      time, median of RUNS runs after WARM warm-up runs; outputs compared with the CPU device
  (b) the node's launch alone on single-node graphs of those shapes, one process, alternating rounds of tamd_graph_profile: d2s_u8 /
      d2s_i8 (TAMD_PIN=d2s_form=1) beside the canonical gather (d2s_form=0; in int8 where it is legal: 16 output channels), and lut_u8
      (a Sigmoid) on the same byte count as the pure-copy yardstick; then the same on larger maps (LARGE), where the forms cross

    python tools/d2s_profile.py [directory of the other build's two libraries]
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

import d2s_helpers as dh  # noqa: E402
import lut_helpers as lh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_INT8, DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 200, 5
TYPES = {"int8": DT_INT8, "uint8": DT_UINT8}
GRAPHS = {
    "EDSR up-sampler, shuffle (1,64,64,64) r 2": lambda dt: dh.edsr_upsampler(dt, dims=(1, 16, 64, 64), r=2),
    "ESPCN tail, shuffle (1,27,120,120) r 3": lambda dt: dh.espcn_tail(dt, dims=(1, 8, 120, 120), r=3, outc=3),
}
# (type, input dims, block size): the launch alone.  (1,144,120,120) r 3 is the int8 shape with 16 output channels, where form 0 is legal
NODES = [("uint8", (1, 64, 64, 64), 2), ("uint8", (1, 27, 120, 120), 3), ("int8", (1, 64, 64, 64), 2), ("int8", (1, 144, 120, 120), 3), ("int8", (1, 27, 120, 120), 3)]
# .. and where the two forms cross: the same shuffles on larger maps, up to a 720p -> 1440p and a 360p -> 1080p output
LARGE = [("uint8", (1, 64, 128, 128), 2), ("uint8", (1, 48, 360, 640), 2), ("uint8", (1, 27, 360, 640), 3), ("int8", (1, 64, 128, 128), 2), ("int8", (1, 64, 256, 256), 2),
         ("int8", (1, 64, 360, 640), 2), ("int8", (1, 144, 240, 240), 3)]


def child(plugin, case, tname):
    """one process, one plugin: prints `placement median_us equal`"""
    from oracle import ref_capi as ref
    import test_plugin_dropin as tp
    tp.PLUGIN = plugin
    tp._load_plugin(ref)
    dt = TYPES[tname]
    g, x = GRAPHS[case](dt)
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, dt)
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
                                                                           " ".join("%.2f" % v for v in vals)))


def through_the_plugin(other):
    mine = os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so")
    sides = [("this plugin", mine)]
    if other:
        sides.insert(0, ("parent plugin", os.path.join(other, "libtengine_hip_device.so")))
    for case in GRAPHS:
        for tname in TYPES:
            res = {s[0]: [] for s in sides}
            placed = {}
            for _ in range(ROUNDS):
                for side, plugin in sides:
                    env = dict(os.environ)
                    env.pop("TAMD_PIN", None)
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", plugin, case, tname], capture_output=True, text=True, timeout=300, env=env)
                    r = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                    if out.returncode != 0 or not r:      # a dead child may have faulted the GPU: nothing more is started on it
                        print("  %s %s %s: child exited with status %d; stopping here.  %s" % (case, tname, side, out.returncode, out.stderr[-300:]))
                        return out.returncode or 1
                    _, pl, us, eq = r[0].split()
                    assert eq == "1", (case, tname, side, "outputs differ from the CPU device")
                    res[side].append(float(us))
                    placed[side] = pl
            print("%s, %s, us per run_graph" % (case, tname))
            for side, _ in sides:
                line("%s: %s" % (side, placed[side]), res[side])
    return 0


def launches(nodes, rounds=9, iters=200):
    """both forms of a node and the yardstick live in this process, timed in alternation, one round of all of them thrown away first;
    us per launch (tamd_graph_profile: eager, one event pair around `iters` back-to-back launches)"""
    ours = ("d2s_u8", "d2s_i8", "transpose_gather_q8", "lut_u8")
    for tname, dims, r in nodes:
        dt = TYPES[tname]
        g, x = dh.d2s_graph(dt, dims, r)
        b = tm2.write_tm2(g)
        graphs = {}
        for name, pin in (("d2s_form=1", "d2s_form=1"), ("d2s_form=0", "d2s_form=0")):
            os.environ["TAMD_PIN"] = pin
            try:
                gr = capi.Graph(b)
            finally:
                os.environ.pop("TAMD_PIN", None)
            gr.set_input(x)
            graphs[name] = (gr, gr.run())
        assert np.array_equal(graphs["d2s_form=1"][1][0], graphs["d2s_form=0"][1][0]) and np.array_equal(graphs["d2s_form=1"][1][0], dh.numpy_d2s(x, r))
        yard = capi.Graph(tm2.write_tm2(lh.unary_graph("Sigmoid", dt, dims, (0.05, 0 if dt == DT_INT8 else 77), (1 / 256.0, 0))))
        yard.set_input(x)
        graphs["Sigmoid on the same bytes"] = (yard, yard.run())
        res = {}
        for k in range(rounds + 1):
            for name, (gr, _) in graphs.items():
                prof = gr.profile(iters)
                if k == 0:
                    continue
                for p in prof:
                    if p["kernel"] in ours:
                        res.setdefault((name, p["kernel"]), []).append(p["ms"] * 1e3)
        print("the launch alone: %s %s r %d, %d bytes" % (tname, dims, r, int(np.prod(dims))))
        for (name, k), v in res.items():
            line("%s: %s" % (name, k), v)
        for gr, _ in graphs.values():
            gr.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4])
        sys.exit(0)
    if capi.device_count() < 1:
        sys.exit("no GPU: nothing is measured")
    if not (len(sys.argv) > 2 and sys.argv[2] == "launches"):
        rc = through_the_plugin(sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None)
        if rc:
            sys.exit(rc)
    launches(NODES)
    launches(LARGE, iters=50)
    sys.exit(0)
