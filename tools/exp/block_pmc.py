#!/usr/bin/env python3
"""HBM traffic of the fused bottleneck launch (block_i8) against the three launches it replaces, per launch, from rocprofv3 --pmc
FETCH_SIZE / WRITE_SIZE passes of their own (counters only), calibrated on tools/exp/hbm_calib.hip as tools/traffic_summary.py does.

  block_pmc.py run <0|1> [model=resnet50] [batch=32] [iters=5]      the target of a counter pass: the model as ONE eager launch list
        (split_batch = 1, no hipGraph), TAMD_FUSE_BLOCK as given; prints the launch list with the planner's algorithmic bytes
  block_pmc.py sum calib_fetch calib_write off_fetch off_write on_fetch on_write off.log on.log
        the trailing iters x (launches + 2) dispatches of every pass are the runs themselves; position in a run = position in the launch
        list (+ 1: the upload launch), so every launch of the fused blocks gets its own counters: counter bytes / algorithmic bytes

(both run ON THE GPU BOX)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def run(fuse, name="resnet50", batch=32, iters=5):
    from tengine_amd import capi, models, tm2
    g = models.build(name, "int8", batch, device_only=True)
    os.environ["TAMD_FUSE_BLOCK"] = fuse
    gr = capi.Graph(tm2.write_tm2(g), batch=batch, use_hip_graph=False, split_batch=1)
    gr.set_input(models.synth_input(g, 3, tm2.DT_INT8))
    steps = gr.profile(1)
    print("launches_per_run %d iters %d" % (gr.kernel_num() + 2, iters))
    for i, k in enumerate(steps):
        print("step %d %s %s %.0f" % (i, k["node"], k["kernel"], k["bytes"]))
    for _ in range(iters):
        gr.run()
    gr.close()


def per_dispatch(d, counter, kernel=""):
    import csv
    import glob
    from collections import defaultdict
    per = defaultdict(float)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter and kernel in r["Kernel_Name"]:
                per[(f, int(r["Dispatch_Id"]))] += float(r["Counter_Value"])
    return [per[k] for k in sorted(per)]


def read_log(path):
    steps, k, iters = [], 0, 0
    for ln in open(path):
        w = ln.split()
        if w[:1] == ["launches_per_run"]:
            k, iters = int(w[1]), int(w[3])
        elif w[:1] == ["step"]:
            steps.append((w[2], w[3], float(w[4])))
    return steps, k, iters


def summarize(cf, cw, of, ow, nf, nw, olog, nlog):
    known = float(1024 << 20)
    unit = {}
    for c, d in (("FETCH_SIZE", cf), ("WRITE_SIZE", cw)):
        v = per_dispatch(d, c, "calib_copy_k")      # the 1 GiB copy launches alone (the program also fills its buffers)
        unit[c] = known / (sum(v) / len(v))
        print("calibration %s: %.1f reported per 1 GiB copy launch -> %.3f bytes per unit" % (c, sum(v) / len(v), unit[c]))
    rows = {}
    for side, fd, wd, log in (("off", of, ow, olog), ("on", nf, nw, nlog)):
        steps, k, iters = read_log(log)
        f, w = per_dispatch(fd, "FETCH_SIZE")[-k * iters:], per_dispatch(wd, "WRITE_SIZE")[-k * iters:]
        assert len(f) == k * iters and len(w) == k * iters and k == len(steps) + 2, (len(f), len(w), k, len(steps))
        rows[side] = []
        for i, (node, kern, alg) in enumerate(steps):
            rd = sum(f[r * k + i + 1] for r in range(iters)) / iters * unit["FETCH_SIZE"]
            wr = sum(w[r * k + i + 1] for r in range(iters)) / iters * unit["WRITE_SIZE"]
            rows[side].append((node, kern, alg, rd, wr))
    print("%-4s %-52s %-34s %10s %10s %10s %7s" % ("side", "node", "kernel", "alg MB", "read MB", "write MB", "ratio"))
    for node, kern, alg, rd, wr in rows["on"]:
        if kern != "block_i8":
            continue
        parts = node.split("+")
        three = [r for r in rows["off"] if r[0] in parts]
        for r in three:
            print("%-4s %-52s %-34s %10.2f %10.2f %10.2f %7.2f" % ("off", r[0], r[1], r[2] / 1e6, r[3] / 1e6, r[4] / 1e6, (r[3] + r[4]) / r[2]))
        a3, r3, w3 = (sum(r[i] for r in three) for i in (2, 3, 4))
        print("%-4s %-52s %-34s %10.2f %10.2f %10.2f %7.2f" % ("off", "  three launches", "", a3 / 1e6, r3 / 1e6, w3 / 1e6, (r3 + w3) / a3))
        print("%-4s %-52s %-34s %10.2f %10.2f %10.2f %7.2f" % ("on", node[:52], kern, alg / 1e6, rd / 1e6, wr / 1e6, (rd + wr) / alg))
    for side in ("off", "on"):
        print("whole launch list, %s: algorithmic %.1f MB, counters %.1f MB read + %.1f MB write"
              % (side, sum(r[2] for r in rows[side]) / 1e6, sum(r[3] for r in rows[side]) / 1e6, sum(r[4] for r in rows[side]) / 1e6))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], *(sys.argv[3:4]), *(int(v) for v in sys.argv[4:6]))
    else:
        summarize(*sys.argv[2:10])
