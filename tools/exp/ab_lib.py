#!/usr/bin/env python3
"""A/B of two BUILDS of libtengine_amd.so on one config's device-resident step, interleaved inside one box: each measurement is a
fresh process that imports a private copy of the tengine_amd package holding the build under test (a process can load the
library only once), plans from its own plan file, checks its bytes against the other build's and times the step as bench.py does.

usage: ab_lib.py model batch dtype iters rounds  NAME=/path/to/libtengine_amd.so  NAME=...   (NAME=product: the tree's own build)
       [env TAMD_U8_INT=1 etc. is inherited; with TAMD_DEBUG=1 each round also shows the planner's "activations: .. buffers share .. MB" line;
        AB_STEP=1 adds the step as bench.py's region times it -- launch() x iters + sync() on the host's clock, where a graph with two slots
        keeps two passes in flight -- and then reads the time_launches figure as the LATENCY column, beside a loop of one launch + sync
        and the blocking run() median; it applies the project's acceptance rule (profiles/chain4_ab.txt) to the last build against the first;
        AB_LAYERS=1 adds per-launch tables (isolated launches, HIP events): the first build beside each other one;
        a worker that dies ends the run with exit status 1: nothing more is started on a GPU that may have faulted]"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKER = r'''
import hashlib, json, os, sys
sys.path.insert(0, os.environ["AB_PKG"])
from tengine_amd import capi, models, tm2
name, batch, dtype, iters = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
g = models.build(name, dtype, batch, device_only=True)
x = models.synth_input(g, 3, {"uint8": tm2.DT_UINT8, "fp32": tm2.DT_FP32}.get(dtype, tm2.DT_INT8))
gr = capi.Graph(tm2.write_tm2(g), batch=batch, direct_dispatch=True)
gr.set_input(x)
out = gr.run()
h = hashlib.sha256(b"".join(o.tobytes() for o in out)).hexdigest()[:16]
gr.upload(); gr.sync()
gr.time_launches(max(3, iters // 10))
ts = [1e3 * gr.time_launches(iters) / iters for _ in range(3)]
extra = {}
if os.environ.get("AB_STEP"):
    # the step as bench.py's region times it: launch() x iters + sync() on the host's clock (a graph with two slots keeps two passes in
    # flight here; time_launches above stays one pass at a time -- the latency column), then the other two latency figures
    import time
    def region():
        t0 = time.perf_counter()
        for _ in range(iters):
            gr.launch()
        gr.sync()
        return 1e6 * (time.perf_counter() - t0) / iters
    region()
    extra["step_us"] = min(region() for _ in range(3))
    def lone(n):
        t0 = time.perf_counter()
        for _ in range(n):
            gr.launch(); gr.sync()
        return 1e6 * (time.perf_counter() - t0) / n
    lone(50)
    extra["lone_us"] = min(lone(max(50, iters // 4)) for _ in range(3))
    gr.run_noreturn(); gr.run_noreturn()
    rs = []
    for _ in range(max(200, iters // 4)):
        t0 = time.perf_counter(); gr.run_noreturn(); rs.append(1e6 * (time.perf_counter() - t0))
    extra["run_us"] = sorted(rs)[len(rs) // 2]
    extra["slots"] = gr.slots()
    gr.upload(); gr.launch(); gr.launch(); gr.launch(); gr.sync()
    extra["sha_launch"] = hashlib.sha256(b"".join(o.tobytes() for o in gr.download())).hexdigest()[:16]
layers = [(k["node"], k["kernel"], k["ms"] * 1e3) for k in gr.profile(max(3, iters // 10))] if os.environ.get("AB_LAYERS") else []
print(json.dumps(dict({"us": min(ts), "sha": h, "launches": gr.kernel_num(), "prerun_ms": gr.prerun_ms(), "layers": layers}, **extra)))
'''


def main():
    name, batch, dtype, iters, rounds = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
    tmp = tempfile.mkdtemp(prefix="ab_lib_")
    variants = []
    for spec in sys.argv[6:]:
        nm, _, path = spec.partition("=")
        pkg = os.path.join(tmp, nm)
        shutil.copytree(os.path.join(ROOT, "tengine_amd"), os.path.join(pkg, "tengine_amd"), ignore=shutil.ignore_patterns("obj", "__pycache__"))
        if path and path != "product":
            shutil.copyfile(path, os.path.join(pkg, "tengine_amd", "lib", "libtengine_amd.so"))
        variants.append((nm, pkg, os.path.join(tmp, nm + "_plan.txt")))
        if os.environ.get("AB_STEP"):                       # as bench.py does: the shipped plan of the configuration seeds every build's plan file
            sys.path.insert(0, ROOT)
            from tengine_amd import plans
            plans.seed(variants[-1][2], name, dtype, int(batch))
    res = {nm: [] for nm, _, _ in variants}
    step = {nm: {"step_us": [], "lone_us": [], "run_us": []} for nm, _, _ in variants}
    slots, sha_launch = {}, {}
    prerun = {nm: [] for nm, _, _ in variants}
    sha = {}
    layers = {}
    for r in range(rounds):
        for nm, pkg, plan in variants:
            env = dict(os.environ, AB_PKG=pkg, TAMD_PLAN_CACHE=plan)
            p = subprocess.run([sys.executable, "-c", WORKER, name, batch, dtype, iters], env=env, capture_output=True, text=True, timeout=900)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode or not line:
                # a dead worker may have faulted the GPU: nothing more is started on it (the machines are shared)
                print("  %s: FAILED (exit status %d), stopping\n%s" % (nm, p.returncode, p.stderr[-800:]))
                shutil.rmtree(tmp, ignore_errors=True)
                sys.exit(1)
            j = json.loads(line[-1])
            res[nm].append(j["us"])
            prerun[nm].append(j["prerun_ms"])
            sha[nm] = j["sha"]
            if "step_us" in j:
                for k in step[nm]:
                    step[nm][k].append(j[k])
                slots[nm], sha_launch[nm] = j["slots"], j["sha_launch"]
                print("  round %d %-20s step %7.2f us | latency: time_launches %7.2f  launch+sync %7.2f  run() median %7.2f | slots %d  sha after launches %s"
                      % (r, nm, j["step_us"], j["us"], j["lone_us"], j["run_us"], j["slots"], j["sha_launch"]), flush=True)
            shared = [l.split("activations: ")[1] for l in p.stderr.splitlines() if l.startswith("[tamd] activations: ")]
            print("  round %d %-20s %9.2f us  %d launches  sha %s  prerun %8.1f ms%s" % (r, nm, j["us"], j["launches"], j["sha"], j["prerun_ms"], "  | " + " / ".join(shared) if shared else ""),
                  flush=True)
            for node, kern, us in j.get("layers", []):
                key = (node, kern)
                layers.setdefault(nm, {})
                layers[nm][key] = min(us, layers[nm].get(key, 1e30))
    print("== %s %s b%s: us per step (direct dispatch), %d fresh processes per build, interleaved; min of 3 x %s steps each" % (name, dtype, batch, rounds, iters))
    for nm, _, _ in variants:
        v = sorted(res[nm])
        if v:
            print("  %-28s min %9.2f  median %9.2f  max %9.2f | output sha %s%s" % (nm, v[0], v[len(v) // 2], v[-1], sha.get(nm), "" if len(set(sha.values())) == 1 else "  (DIFFERS between builds)"))
    if all(step[nm]["step_us"] for nm, _, _ in variants):
        def mmm(v):
            v = sorted(v)
            return v[0], v[len(v) // 2], v[-1]
        print("  -- the step as bench.py times it (launch() x %s + sync(), host clock), and the latency figures; us, min / median / max over the rounds" % iters)
        for nm, _, _ in variants:
            print("  %-20s slots %d | step %s | time_launches %s | launch+sync %s | run() %s | sha after launches %s%s" % (
                nm, slots[nm], " / ".join("%.2f" % x for x in mmm(step[nm]["step_us"])), " / ".join("%.2f" % x for x in mmm(res[nm])),
                " / ".join("%.2f" % x for x in mmm(step[nm]["lone_us"])), " / ".join("%.2f" % x for x in mmm(step[nm]["run_us"])), sha_launch[nm],
                "" if len(set(sha_launch.values())) == 1 else "  (DIFFERS between builds)"))
        if len(variants) > 1:
            a, b = variants[0][0], variants[-1][0]
            sa, sb = mmm(step[a]["step_us"]), mmm(step[b]["step_us"])
            spread = max(sa[2] - sa[0], sb[2] - sb[0])
            print("  decision (%s against %s): median step %.2f -> %.2f us, %.2f us lower (%+.1f %% images/s); three times the larger min-max spread = %.2f us: the rule is %s"
                  % (b, a, sa[1], sb[1], sa[1] - sb[1], 100.0 * (sa[1] / sb[1] - 1.0), 3 * spread, "MET" if sa[1] - sb[1] > 3 * spread else "NOT met"))
            for key, label in (("us", "time_launches"), ("lone_us", "launch+sync"), ("run_us", "run() median")):
                va, vb = (mmm(res[a]), mmm(res[b])) if key == "us" else (mmm(step[a][key]), mmm(step[b][key]))
                sp = max(va[2] - va[0], vb[2] - vb[0])
                print("  latency %-14s median %.2f -> %.2f us (%+.2f), larger spread %.2f: %s" % (label, va[1], vb[1], vb[1] - va[1], sp, "not worse beyond the spread" if vb[1] - va[1] <= sp else "WORSE beyond the spread"))
    for nm, _, _ in variants:                              # round 0 times the plan-time races, the later rounds take its plan file
        v = sorted(prerun[nm][1:])
        if v:
            print("  %-28s prerun_ms, rounds 1..: min %8.1f  median %8.1f  max %8.1f   (round 0, racing: %.1f)" % (nm, v[0], v[len(v) // 2], v[-1], prerun[nm][0]))
    for other in variants[1:] if layers else []:          # AB_LAYERS=1: isolated launches (HIP events), min over the rounds, the first build beside each other one
        a, b = variants[0][0], other[0]
        print("  per launch, isolated (us): %-24s %-34s %8s | %-34s %8s" % ("node", a, "", b, ""))
        nodes = []
        for nm in (a, b):
            for (node, kern) in layers.get(nm, {}):
                if node not in nodes:
                    nodes.append(node)
        for node in nodes:
            ea = sorted((us, k) for (n, k), us in layers.get(a, {}).items() if n == node)
            eb = sorted((us, k) for (n, k), us in layers.get(b, {}).items() if n == node)
            if ea and eb:
                print("    %-38s %-34s %8.2f | %-34s %8.2f  %+6.1f%%" % (node[:38], ea[0][1][:34], ea[0][0], eb[0][1][:34], eb[0][0], 100 * (eb[0][0] / ea[0][0] - 1)))
            elif ea or eb:                                  # a node one build runs inside another launch (a fused chain): listed on its own side
                e = (ea or eb)[0]
                print("    %-38s %-34s %8s | %-34s %8s" % ((node[:38], e[1][:34], "%.2f" % e[0], "-", "") if ea else (node[:38], "-", "", e[1][:34], "%.2f" % e[0])))
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
