#!/usr/bin/env python3
"""The measurements behind profiles/slice_u8.txt (runs ON THE GPU BOX, prints the tables):

  (a) a YOLOv4-tiny CSP block at (1,64,104,104) and YOLOv5's Focus graph at (1,3,640,640) through the plugin -- create_graph / prerun_graph /
      run_graph of the unmodified reference library on device "HIP" -- with the plugin of ANOTHER build (the parent commit: the directory
      given as argument holds its libtengine_hip_device.so and libtengine_amd.so) and with this tree's, one child process per run, the two
      in alternation; host to host run_graph time, median of RUNS runs after WARM warm-up runs; outputs compared with the CPU device
  (b) slice_u8 beside its neighbours on the same bytes, one process, alternating rounds of tamd_graph_profile: a channel range of
      (8,128,52,52) [batch 1 for the uint8 Split, which the reference defines there only] against chan_map_u8 doing the same Split;
      W step 2 on (1,3,640,640) with the two-load path and byte by byte (TAMD_PIN=slice_w2=0); the chain of two Slices fused and as two
      launches (TAMD_PIN=slice_chain=0)

    python tools/slice_profile.py [directory of the other build's two libraries]
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

import slice_op_helpers as so  # noqa: E402
import shuffle_helpers as sh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_UINT8  # noqa: E402

WARM, RUNS, ROUNDS = 20, 200, 5
BLOCKS = {"csp": lambda: so.csp_graph((1, 64, 104, 104), 64), "focus": lambda: so.focus_graph((1, 3, 640, 640), 32)}


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
    print("  %-44s median %8.2f  min %8.2f  max %8.2f  spread %6.2f | %s" % (name, statistics.median(vals), min(vals), max(vals), max(vals) - min(vals),
                                                                           " ".join("%.2f" % v for v in vals)))


def blocks(other):
    mine = os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so")
    for case in BLOCKS:
        res = {"parent": [], "this": []}
        placed = {}
        for _ in range(ROUNDS):
            for side, plugin in (("parent", os.path.join(other, "libtengine_hip_device.so")), ("this", mine)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", plugin, case], capture_output=True, text=True, timeout=300)
                r = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
                if out.returncode != 0 or not r:          # a dead child may have faulted the GPU: nothing more is started on it
                    print("  %s %s: child exited with status %d; stopping here.  %s" % (case, side, out.returncode, out.stderr[-300:]))
                    return out.returncode or 1
                _, pl, us, eq = r[0].split()
                assert eq == "1", (case, side, "outputs differ from the CPU device")
                res[side].append(float(us))
                placed[side] = pl
        g, _ = BLOCKS[case]()
        print("%s, input %s" % (case, tuple(g.tensors[0].dims)))
        for side in ("parent", "this"):
            line("%s plugin: %s" % (side, placed[side]), res[side])
    return 0


def one_launch_us(builds, rounds=9, iters=200):
    """builds: {name: (tm bytes, input, TAMD_PIN or None, kernel name)}; every graph lives in this process, timed in alternation, one
    round of all of them thrown away first; the figure of a graph is the sum over its launches of that kernel, us per launch
    (tamd_graph_profile: eager, one event pair around `iters` back-to-back launches)"""
    graphs = {}
    for name, (b, x, pin, kernel) in builds.items():
        if pin:
            os.environ["TAMD_PIN"] = pin
        try:
            gr = capi.Graph(b)
        finally:
            os.environ.pop("TAMD_PIN", None)
        gr.set_input(x)
        out = gr.run()
        graphs[name] = (gr, kernel, out)
    res = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for name, (gr, kernel, _) in graphs.items():
            prof = gr.profile(iters)
            if r == 0:
                continue
            hit = [k["ms"] * 1e3 for k in prof if k["kernel"].startswith(kernel)]
            assert hit, (name, [(k["node"], k["kernel"]) for k in prof])
            res[name].append(hit[-1] if kernel == "chan_map_u8" else sum(hit))        # (the Split's second output: the same planes)
    for name in graphs:
        line(name, res[name])
    outs = {k: v[2] for k, v in graphs.items()}
    for gr, _, _ in graphs.values():
        gr.close()
    return outs


def kernels():
    q = so.IN_Q
    for n in (1, 8):
        dims = (n, 128, 52, 52)
        print("channel range [64,128) of %s, %d bytes out, requantised 0.05/77 -> 0.031/12 and between equal parameters" % (dims, n * 64 * 52 * 52))
        builds = {}
        for tag, oq in (("requant", so.OUT_Q), ("identity", q)):
            g, x = so.slice_graph(dims, 1, 64, 128, out_q=oq)
            builds["slice_u8 %s" % tag] = (tm2.write_tm2(g), x, None, "slice_u8")
            if n == 1:          # the uint8 Split is defined for batch 1 only
                g, x2 = sh.split_graph(DT_UINT8, dims, [64, 64], in_q=q, out_qs=[q, oq], cat_q=oq)
                builds["chan_map_u8 %s (Split [64,64], output 1)" % tag] = (tm2.write_tm2(g), x2, None, "chan_map_u8")
        one_launch_us(builds)
    print("W step 2 of (1,3,640,640) -> (1,3,640,320), begin 0 and 1")
    builds = {}
    for begin in (0, 1):
        g, x = so.slice_graph((1, 3, 640, 640), 3, begin, 640, 2)
        b = tm2.write_tm2(g)
        builds["two loads + permutes, begin %d" % begin] = (b, x, None, "slice_u8")
        builds["byte by byte (slice_w2=0), begin %d" % begin] = (b, x, "slice_w2=0", "slice_u8")
    outs = one_launch_us(builds)
    for begin in (0, 1):
        assert np.array_equal(outs["two loads + permutes, begin %d" % begin][0], outs["byte by byte (slice_w2=0), begin %d" % begin][0])
    print("chain Slice(axis 2, begin 1, step 2) -> Slice(axis 3, begin 0, step 2) of (1,3,640,640)")
    g, x = so.chain_graph((1, 3, 640, 640))
    b = tm2.write_tm2(g)
    outs = one_launch_us({"fused, one launch": (b, x, None, "slice_u8"), "two launches (slice_chain=0), their sum": (b, x, "slice_chain=0", "slice_u8")})
    assert np.array_equal(outs["fused, one launch"][0], outs["two launches (slice_chain=0), their sum"][0])


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    if capi.device_count() < 1:
        sys.exit("no GPU: nothing is measured")
    rc = 0
    if len(sys.argv) > 1:
        rc = blocks(sys.argv[1])
        if rc:
            sys.exit(rc)
    else:
        print("(no other build given: the block timings are skipped)")
    kernels()
    sys.exit(rc)
