#!/usr/bin/env python3
"""The measurements behind profiles/resize.txt (runs ON THE GPU BOX, prints the tables):

  (a) the up-sampling neck through the plugin -- create_graph / prerun_graph / run_graph of the unmodified reference library on device
      "HIP" -- in int8 and uint8: skip = conv1x1(data); low = conv1x1(maxpool 2/2 (data)); Resize x2 (low); Concat([up, skip]) ->
      conv1x1, with the Resize on (1,128,20,20) and on (1,256,40,40) (tests/resize_helpers.py: neck_block).  Three sides, one child
      process per run, in alternation: the plugin of ANOTHER build (the parent commit: the directory given as argument holds its
      libtengine_hip_device.so and libtengine_amd.so), which leaves the node to the CPU device, and this tree's with
      TAMD_PIN=resize_form=0 and =1.  Host to host run_graph time, median of RUNS runs after WARM warm-up runs; outputs compared with
      the CPU device
  (b) the node's launch alone on single-node graphs of those shapes and of one large tensor (4 MiB of output and more), one process,
      alternating rounds of tamd_graph_profile: resize_rep_i8 / resize_rep_u8 (resize_form=1) beside interp_nearest_i8 /
      interp_nearest_u8 fed with Resize's operands (resize_form=0), and lut_u8 (a Sigmoid) on the OUTPUT's byte count as the
      pure-copy yardstick

    python tools/resize_profile.py [directory of the other build's two libraries | -] [launches]
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

import lut_helpers as lh  # noqa: E402
import resize_helpers as rh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_INT8, DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 200, 3
TYPES = {"int8": DT_INT8, "uint8": DT_UINT8}
GRAPHS = {
    "neck, Resize x2 of (1,128,20,20)": lambda dt: rh.neck_block(dt, dims=(1, 128, 20, 20), cmid=128, cskip=128, cout=128, k=1),
    "neck, Resize x2 of (1,256,40,40)": lambda dt: rh.neck_block(dt, dims=(1, 256, 40, 40), cmid=256, cskip=256, cout=256, k=1),
}
# (type, input dims, (scale_h, scale_w)): the launch alone
NODES = [("int8", (1, 128, 20, 20), (2.0, 2.0)), ("uint8", (1, 128, 20, 20), (2.0, 2.0)), ("int8", (1, 256, 40, 40), (2.0, 2.0)), ("uint8", (1, 256, 40, 40), (2.0, 2.0)),
         ("int8", (1, 64, 128, 128), (2.0, 2.0)), ("uint8", (1, 64, 128, 128), (2.0, 2.0)), ("int8", (1, 256, 80, 80), (2.0, 2.0)), ("uint8", (1, 256, 80, 80), (2.0, 2.0)),
         ("uint8", (1, 64, 128, 128), (3.0, 3.0))]


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
    sides = [("this plugin, resize_form=0", mine, "resize_form=0"), ("this plugin, resize_form=1", mine, "resize_form=1")]
    if other:
        sides.insert(0, ("parent plugin", os.path.join(other, "libtengine_hip_device.so"), None))
    for case in GRAPHS:
        for tname in TYPES:
            res = {s[0]: [] for s in sides}
            placed = {}
            for _ in range(ROUNDS):
                for side, plugin, pin in sides:
                    env = dict(os.environ)
                    env.pop("TAMD_PIN", None)
                    if pin:
                        env["TAMD_PIN"] = pin
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", plugin, case, tname], capture_output=True, text=True, timeout=300, env=env)
                    r = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                    if out.returncode != 0 or not r:      # a dead child may have faulted the GPU: nothing more is started on it
                        print("  %s %s %s: child exited with status %d; stopping here.  %s" % (case, tname, side, out.returncode, out.stderr[-300:]))
                        return out.returncode or 1
                    _, pl, us, eq = r[0].split()
                    assert eq == "1", (case, tname, side, "outputs differ from the CPU device")
                    res[side].append(float(us))
                    placed[side] = pl
            print("%s, %s, us per run_graph" % (case, tname), flush=True)
            for side, _, _ in sides:
                line("%s: %s" % (side, placed[side]), res[side])
    return 0


def launches(nodes, rounds=7, iters=200):
    """both forms of a node and the yardstick live in this process, timed in alternation, one round of all of them thrown away first;
    us per launch (tamd_graph_profile: eager, one event pair around `iters` back-to-back launches)"""
    ours = ("resize_rep_i8", "resize_rep_u8", "interp_nearest_i8", "interp_nearest_u8", "lut_u8")
    for tname, dims, sc in nodes:
        dt = TYPES[tname]
        p = rh.scales(*sc)
        g, x = rh.single(dt, dims, p, 5)
        b = tm2.write_tm2(g)
        graphs = {}
        for pin in ("resize_form=1", "resize_form=0"):
            os.environ["TAMD_PIN"] = pin
            try:
                gr = capi.Graph(b)
            finally:
                os.environ.pop("TAMD_PIN", None)
            gr.set_input(x)
            graphs[pin] = (gr, gr.run())
        q = (rh.IN_Q[dt], rh.OUT_Q[dt])
        want = rh.numpy_resize(x, p, capi.resize_table(dt, lh.f32(q[0][0]), q[0][1], lh.f32(q[1][0]), q[1][1]))
        assert np.array_equal(graphs["resize_form=1"][1][0], want) and np.array_equal(graphs["resize_form=0"][1][0], want)
        ydims = want.shape
        yard = capi.Graph(tm2.write_tm2(lh.unary_graph("Sigmoid", dt, ydims, (0.05, 0 if dt == DT_INT8 else 77), (1 / 256.0, 0))))
        yard.set_input(lh.random_bytes(3, dt, ydims))
        graphs["Sigmoid on the output's bytes"] = (yard, yard.run())
        res = {}
        for k in range(rounds + 1):
            for name, (gr, _) in graphs.items():
                prof = gr.profile(iters)
                if k == 0:
                    continue
                for pr in prof:
                    if pr["kernel"] in ours:
                        res.setdefault((name, pr["kernel"]), []).append(pr["ms"] * 1e3)
        print("the launch alone: %s %s x(%g, %g), %d bytes in, %d bytes out" % (tname, dims, sc[0], sc[1], int(np.prod(dims)), int(np.prod(ydims))), flush=True)
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
    sys.exit(0)
