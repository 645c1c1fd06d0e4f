#!/usr/bin/env python3
"""The measurements behind profiles/transpose.txt (runs ON THE GPU BOX, prints the tables):

  (a) the Detect head of the YOLOv5 family at its real shapes -- conv1x1 (32 -> 255) -> Reshape (1,3,85,H,W) -> Transpose (0,1,3,4,2) ->
      Sigmoid -> Reshape (1,3*H*W,85) at H = W = 80, 40, 20, int8 and uint8 -- through the plugin: create_graph / prerun_graph / run_graph
      of the unmodified reference library on device "HIP", with the plugin of ANOTHER build (the parent commit: the directory given as
      argument holds its libtengine_hip_device.so and libtengine_amd.so) and with this tree's, one child process per run, the two in
      alternation; host to host run_graph time, median of RUNS runs after WARM warm-up runs; outputs compared with the CPU device
  (b) the kernels alone, per launch, one process each, alternating rounds of tamd_graph_profile: transpose_tile_q8 against
      transpose_gather_q8 (TAMD_PIN=transpose_form=0) at (1,3,85,6400) order (0,1,3,2) and at NCHW -> NHWC (1,256,40,40);
      transpose_rows_q8 against the gather at the int8 head read from NHWC; lut_u8 (a Sigmoid) on the same byte count beside them, the
      floor of one read and one write
  (c) the int8 head with the view form (one launch) and with TAMD_PIN=transpose_view=0 (reshape_i8 + transpose), the whole launch list

    python tools/transpose_profile.py [--part a|b|c] [directory of the other build's two libraries]
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
import transpose_helpers as th  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_INT8, DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 200, 4
DT = {"i8": DT_INT8, "u8": DT_UINT8}


def head_graph(dtype, side, cin=32):
    """one scale of the Detect head at its real width: 3 anchors x 85 values"""
    c = th.Block(71, dtype, (1, cin, side, side))
    c.conv(255, 1)
    c.reshape((1, 3, 85, side, side))
    c.transpose((0, 1, 3, 4, 2), out_q=(c.scale() * 0.7, 0 if dtype == DT_INT8 else 140))
    c.act("Sigmoid")
    c.reshape((1, 3 * side * side, 85))
    return c.done()


def child(plugin, tag, side):
    """one process, one plugin: prints `placement median_us equal`"""
    from oracle import ref_capi as ref
    import test_plugin_dropin as tp
    tp.PLUGIN = plugin
    tp._load_plugin(ref)
    g, x = head_graph(DT[tag], side)
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, DT[tag])
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


def blocks(other):
    mine = os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so")
    for tag in ("i8", "u8"):
        for side in (80, 40, 20):
            res = {"parent": [], "this": []}
            placed = {}
            for _ in range(ROUNDS):
                for who, plugin in (("parent", os.path.join(other, "libtengine_hip_device.so")), ("this", mine)):
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", plugin, tag, str(side)], capture_output=True, text=True, timeout=300)
                    r = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                    if out.returncode != 0 or not r:      # a dead child may have faulted the GPU: nothing more is started on it
                        print("  %s %d %s: child exited with status %d; stopping here.  %s" % (tag, side, who, out.returncode, out.stderr[-300:]))
                        return out.returncode or 1
                    _, pl, us, eq = r[0].split()
                    assert eq == "1", (tag, side, who, "outputs differ from the CPU device")
                    res[who].append(float(us))
                    placed[who] = pl
            print("Detect head %s, conv output (1,255,%d,%d): run_graph us, one figure per process" % (tag, side, side))
            for who in ("parent", "this"):
                line("%s plugin: %s" % (who, placed[who]), res[who])
    return 0


def one_launch_us(builds, rounds=7, iters=200):
    """builds: {name: (tm bytes, input, TAMD_PIN or None, kernel name or None for the whole list)}; every graph lives in this process, timed
    in alternation, one round of all of them thrown away first; us per launch (tamd_graph_profile: eager, one event pair around `iters`
    back-to-back launches), summed over the launches of that kernel (None: over the whole launch list)"""
    graphs = {}
    for name, (b, x, pin, kernel) in builds.items():
        if pin:
            os.environ["TAMD_PIN"] = pin
        try:
            gr = capi.Graph(b)
        finally:
            os.environ.pop("TAMD_PIN", None)
        gr.set_input(x)
        graphs[name] = (gr, kernel, gr.run())
    res = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for name, (gr, kernel, _) in graphs.items():
            prof = gr.profile(iters)
            if r == 0:
                continue
            hit = [k["ms"] * 1e3 for k in prof if kernel is None or k["kernel"].startswith(kernel)]
            assert hit, (name, [(k["node"], k["kernel"]) for k in prof])
            res[name].append(sum(hit))
    for name in graphs:
        line(name, res[name])
    outs = {k: v[2] for k, v in graphs.items()}
    for gr, _, _ in graphs.values():
        gr.close()
    return outs


def same(outs):
    first = next(iter(outs.values()))
    for v in outs.values():
        assert all(np.array_equal(a, b) for a, b in zip(first, v))


def lut_graph(dtype, dims):
    return lh.unary_graph("Sigmoid", dtype, dims, (0.05, 0 if dtype == DT_INT8 else 77), (1 / 256.0, 0)), lh.random_bytes(3, dtype, dims)


def kernels():
    for dims, order, what in (((1, 3, 85, 6400), (0, 1, 3, 2), "the uint8 head's move, (1,3,85,6400) order (0,1,3,2)"),
                              ((1, 256, 40, 40), (0, 2, 3, 1), "NCHW -> NHWC, (1,256,40,40) order (0,2,3,1)")):
        n = int(np.prod(dims))
        print("%s, %d bytes, uint8, requantised 0.05/77 -> 0.031/12" % (what, n))
        g, x = th.transpose_graph(DT_UINT8, dims, order)
        b = tm2.write_tm2(g)
        gl, xl = lut_graph(DT_UINT8, dims)
        same_out = one_launch_us({"transpose_tile_q8": (b, x, "transpose_form=2", "transpose_tile_q8"),
                                  "transpose_gather_q8 (transpose_form=0)": (b, x, "transpose_form=0", "transpose_gather_q8")})
        same(same_out)
        one_launch_us({"lut_u8 on the same byte count": (tm2.write_tm2(gl), xl, None, "lut_u8")})
    for dims, order, what in (((1, 2, 58, 28, 28), (0, 2, 1, 3, 4), "torch's channel shuffle, (1,2,58,28,28) order (0,2,1,3,4): runs of 784 bytes"),
                              ((8, 3, 85, 6400), (0, 1, 3, 2), "the uint8 head's move at batch 8, (8,3,85,6400) order (0,1,3,2)")):
        print("%s, %d bytes, uint8" % (what, int(np.prod(dims))))
        g, x = th.transpose_graph(DT_UINT8, dims, order)
        b = tm2.write_tm2(g)
        pin = "transpose_form=1" if len(dims) == 5 else "transpose_form=2"
        same(one_launch_us({pin: (b, x, pin, "transpose_"), "transpose_gather_q8 (transpose_form=0)": (b, x, "transpose_form=0", "transpose_gather_q8")}))
    for side in (80, 20):
        print("the int8 head read from NHWC: conv (1,255,%d,%d), 256-byte pixels -> Reshape -> Transpose (0,1,3,4,2), %d bytes" % (side, side, 255 * side * side))
        g, x = head_graph(DT_INT8, side)
        b = tm2.write_tm2(g)
        same(one_launch_us({"transpose_rows_q8 (through the Reshape)": (b, x, "transpose_form=1", "transpose_rows_q8"),
                            "transpose_gather_q8 (transpose_form=0)": (b, x, "transpose_form=0", "transpose_gather_q8"),
                            "lut_u8 behind it, the same byte count": (b, x, None, "lut_u8")}))


def views():
    for side in (80, 40, 20):
        print("int8 Detect head, conv output (1,255,%d,%d): the whole launch list, us per pass" % (side, side))
        g, x = head_graph(DT_INT8, side)
        b = tm2.write_tm2(g)
        same(one_launch_us({"view form: reshape+transpose one launch": (b, x, None, None),
                            "transpose_view=0: reshape_i8 + transpose": (b, x, "transpose_view=0", None)}))
        same(one_launch_us({"view form, the transpose alone": (b, x, None, "transpose_"),
                            "transpose_view=0, reshape_i8 alone": (b, x, "transpose_view=0", "reshape_i8"),
                            "transpose_view=0, the transpose alone": (b, x, "transpose_view=0", "transpose_")}))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--child":
        child(args[1], args[2], int(args[3]))
        sys.exit(0)
    if capi.device_count() < 1:
        sys.exit("no GPU: nothing is measured")
    part = "abc"
    if args and args[0] == "--part":
        part, args = args[1], args[2:]
    rc = 0
    if "a" in part:
        if args:
            rc = blocks(args[0])
            if rc:
                sys.exit(rc)
        else:
            print("(no other build given: the plugin timings are skipped)")
    if "b" in part:
        kernels()
    if "c" in part:
        views()
    sys.exit(rc)
