#!/usr/bin/env python3
"""bench.py -- images/sec of int8 MobileNet-v1 224x224 on N MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
                                                     (N>1: launched by torch.distributed.run, one rank per GPU)

A "step" = one forward pass of the hot path over one batch (default batch 1 = BASELINE configs[1]) of
synthetic int8 input that is already resident in HBM.  Weights: the seeded synthetic int8 model written
as a real tmfile; at N>1 rank 0 RCCL-broadcasts the tmfile bytes once (north_star), every rank loads them
with the native loader, the images are sharded (each rank owns its own batch, weak scaling); a step needs no
collective (independent images, outputs resident in each rank's HBM as at N = 1): every output of the LAST step is
all-gathered once over RCCL inside the timed region (--gather every: one overlapped all_gather per step instead).
Each step is one pass over the graph's launch list, dispatched directly as AQL packets on the graph's own HSA
queue (tamd_options.direct_dispatch, csrc/direct.cc; --direct 0 / --streams > 1 / a profiler attached: hipGraph replay).

Timing: W untimed warm-up steps, then exactly K steps bracketed by barrier + torch.cuda.synchronize() on
both sides, MAX over ranks.  value = N * batch * K / t, ms_per_step = 1e3 * t / K.

A plain run does only that: set-up, warm-up, the one timed region, --dump-outputs, the JSON line.  --dump-outputs DIR
writes every output of the last timed step as DIR/output<i>.npy in float32; inputs and weights are seeded, so two builds
can be compared output for output.  At N > 1 these are rank 0's own outputs (its shard of the batch), not the tensor the
per-step all_gather assembles from every rank.

--full adds everything else, as separate measurements after the headline region: the region repeated until
--min-seconds (the line then reports the MEDIAN region), at N > 1 the no-collective and gather-final regions, at N = 1
the hipGraph-replay region and the other BASELINE configurations (--configs), output sha256 against the reference's
golden, and these extra objects:
  roofline      dominant kernel family, algorithmic bytes / average launch duration measured with HIP
                events on the launch stream in this same process (tamd_graph_profile), vs the HBM peak;
                roofline.direct_dispatch: the same with the launch's cost read off the direct step's clock
  host_to_host  the blocking tamd_graph_run (what tm_benchmark times) and the two-in-flight asynchronous pair
  cpu_baseline  the REAL reference CPU backend (oracle/_ref, built from the unmodified sources) timed on
                this host's cores on a bounded sample (rank 0, N=1 only); falls back to the C oracle port
"""
import argparse
import ctypes
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)
MFMA_I8_PEAK_TOPS = 5000.0   # dense int8 MFMA peak (2x bf16 2.5 PF)
MFMA_F32_PEAK_TOPS = 157.3   # fp32 MFMA peak (the uint8 configs are fp32-simulated: u8_kernels.hip)


class _CAI:
    """Expose a raw device pointer to torch through __cuda_array_interface__ (zero copy)."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1, help="images per GPU per step (BASELINE configs[1]: 1)")
    ap.add_argument("--model", default="mobilenet_v1")
    ap.add_argument("--dtype", default="int8", choices=["int8", "uint8"],
                    help="int8 = BASELINE metric; uint8 = the fp32-simulated configs (yolov3_tiny ...), side lines only")
    ap.add_argument("--u8-integer", action="store_true",
                    help="uint8 models on the opt-in integer path (tamd_options.u8_integer: exact int32 sums on the int8 MFMA, results within "
                         "one quantisation step of the reference per layer instead of byte-identical); a side line, never the default")
    ap.add_argument("--streams", type=int, default=1, help="concurrent batch-1 graph instances (1 = sequential, tm_benchmark semantics)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-dist", action="store_true", help="run the multi-rank code path with world_size 1 (test)")
    ap.add_argument("--cpu-seconds", type=float, default=16.0)
    ap.add_argument("--global-batch", type=int, default=0,
                    help="total images per step, sharded over the ranks with shard_range (strong split of one batch, e.g. "
                         "--model yolov3_tiny --dtype uint8 --global-batch 64); 0 = --batch per GPU (weak scaling)")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU/gloo plumbing check of the N-rank path (spawn, tmfile broadcast, sharding, gather of every "
                         "output); no device work, the JSON line carries value null and dry_run true")
    ap.add_argument("--gather", choices=["both", "final", "every"], default="both",
                    help="N > 1.  every: one all_gather of every output per step, overlapped with the next step (SURVEY 8(e)'s per-batch "
                         "gather; hipGraph replay).  final: no per-step collective (independent images, outputs stay resident in each rank's "
                         "HBM as at N = 1), every output of the LAST step all-gathered once, inside the timed region (direct dispatch).  "
                         "both (default): two timed regions of K steps each, `value` = every, `gather_final` = final as a side object")
    ap.add_argument("--direct", type=int, choices=[0, 1], default=1,
                    help="1 (default): tamd_graph_launch dispatches the launch list as AQL packets on the graph's own HSA queue "
                         "(tamd_options.direct_dispatch, csrc/direct.cc); 0: hipGraph replay on the graph's HIP stream.  "
                         "the per-step gather region (--gather every) awaits each pass on the queue's signal and gathers on a side stream")
    ap.add_argument("--master-port", type=int, default=0)
    ap.add_argument("--min-seconds", type=float, default=0.05,
                    help="--full: the timed region of exactly K steps (barrier + synchronize on both sides, MAX over ranks) is REPEATED until the "
                         "regions add up to this many seconds; the line reports the MEDIAN region (value, ms_per_step) and min / max beside "
                         "it.  The driver's K = 20 is a 1 ms region at batch 1: one scheduling hiccup was a 5 %% swing on the judged number")
    ap.add_argument("--max-repeats", type=int, default=400)
    ap.add_argument("--full", action="store_true",
                    help="after the headline region, also measure and check everything else (region repeats up to --min-seconds, the "
                         "side regions and --configs, roofline, host-to-host, CPU baseline, golden sha256); a plain run times K steps once")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write every output of the last timed step (rank 0) as DIR/output<i>.npy in float32 (at most 64 MB in all; a "
                         "larger set is cut to a fixed seeded sample of each output)")
    ap.add_argument("--configs", default="auto",
                    help="--full, N = 1: also time the other BASELINE configurations in this process, each on its shipped plan, >= 200 steps, no CPU "
                         "baseline, and print them under `configs` (ms_per_step, roofline, output sha256 against tests/golden/"
                         "bench_outputs_sha256.json).  auto = when the headline workload (mobilenet_v1 int8 batch 1) is what runs; none; all")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be at least 1")
    if args.u8_integer:
        if args.dtype != "uint8":
            raise SystemExit("bench.py: --u8-integer is a mode of the uint8 models")
        os.environ["TAMD_U8_INT"] = "1"          # every graph of this job (and of the ranks it spawns)

    # `python bench.py --gpus N` run plainly: start the N ranks ourselves (one process per GPU) -- or fail
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn(args)
        return

    import numpy as np
    import torch

    from tengine_amd import capi, models, plans, tm2

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # every graph of this process (second timed region, concurrent streams) takes the plan the first one measured: the same kernels in
    # every region, one plan-time autotune instead of one per graph (csrc/plan_cache.hip)
    plan_tmp = None
    shipped_plan = None
    if "TAMD_PLAN_CACHE" not in os.environ:
        import tempfile
        plan_tmp = os.path.join(tempfile.gettempdir(), "tamd_plan_%d_%d.txt" % (os.getpid(), rank))
        os.environ["TAMD_PLAN_CACHE"] = plan_tmp
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE %d -- refusing to report a line for the wrong GPU count" % (args.gpus, world))
    if args.dry_run:
        return dry_run(args, rank, world)
    if torch.cuda.device_count() < max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world))):
        raise SystemExit("bench.py: %d rank(s) on this node but %d HIP device(s) visible" % (world, torch.cuda.device_count()))
    use_dist = world > 1 or args.force_dist   # --force-dist exercises the RCCL path on a single GPU (testing)
    dist = None
    torch.cuda.set_device(local_rank)
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    from tengine_amd import dist as tdist
    if args.global_batch:
        args.batch = tdist.shard_range(args.global_batch, world, rank)[1]       # this rank's contiguous shard
        if args.batch == 0:
            raise SystemExit("bench.py: --global-batch %d leaves rank %d without images" % (args.global_batch, rank))
    total_images = args.global_batch if args.global_batch else world * args.batch
    if plan_tmp:
        # the plan the committed evidence was taken with (tengine_amd/plans/, written by tools/make_plans.py on the GPU box): a COPY
        # seeds this job's plan file, so the driver's run launches the kernels the layer tables name instead of re-rolling the
        # plan-time autotune.  The library ignores the file as a whole when its header names another build or candidate list, and
        # re-checks every cached choice before using it (csrc/plan_cache.hip); layers the file does not hold are timed as usual.
        shipped_plan = plans.seed(plan_tmp, args.model, args.dtype + ("_int" if args.u8_integer else ""), args.batch)
    max_shard = tdist.shard_range(total_images, world, 0)[1]

    # ---- model: rank 0 synthesises the int8 tmfile, RCCL broadcast of the raw bytes ----------------
    if rank == 0:
        # the benchmark graph as tm_benchmark runs it, classifier Softmax included (ResNet-50 int8: softmax_i8 since round 4)
        g = models.build(args.model, args.dtype, args.batch)
        tm_bytes = tm2.write_tm2(g)
    if use_dist:
        # RCCL over xGMI, once, outside the timed loop (tengine_amd/dist.py; gloo-tested on CPU)
        tm_bytes = tdist.broadcast_tmfile(tm_bytes if rank == 0 else None, dist, "cuda")
    g = tm2.read_tm2(tm_bytes)

    # S graph instances on S HIP streams: independent batch-1 requests in flight concurrently (serving mode).
    # Default S=1 == tm_benchmark's semantics (one blocking run_graph after the other).
    S = max(1, args.streams)
    u8 = args.dtype == "uint8"
    x = models.synth_input(g, 1000 + rank, tm2.DT_UINT8 if u8 else tm2.DT_INT8)   # each rank owns its own shard of images

    def region(mode, direct, keep=False):
        """One timed region: W warm-up steps, K timed steps, bracketed by barrier + synchronize, MAX over ranks.
        mode: "none" (no collective: N = 1), "final" (every output of the LAST step all-gathered once, inside the region),
        "every" (one all_gather of every output per step, double-buffered on a side stream so it overlaps the next step --
        SURVEY 8(e)'s per-batch gather).  With direct dispatch the passes are not on a HIP stream: step k is awaited on the
        queue's completion signal (tamd_graph_sync), its outputs are copied into the gather slot on the side stream, and the
        next pass is submitted once that copy is done -- the SAME dispatch path as the N = 1 `value`, plus what a per-step
        gather needs (round 5; until round 4 this region replayed hipGraphs and N = 1 / N > 1 timed different paths)."""
        # one HSA queue per graph: with several batch-1 streams the extra queues oversubscribe the hardware queues (measured: 4
        # streams 8.2 k img/s direct against 27.3 k on HIP streams), so the concurrent-streams mode stays on hipGraph replay
        direct = bool(direct) and S == 1
        # a per-step / final all-gather copies out of PERSISTENT views of the outputs' device buffers on the graph's own stream: a graph compiled
        # as two half-batch device graphs has two streams and gathers its outputs only inside tamd_graph_output_device, so the gather regions
        # (N > 1) keep the one-launch-list form; the N = 1 region takes the library's default form (tamd_options.split_batch = 0)
        grs = [capi.Graph(tm_bytes, batch=args.batch, gpu_index=local_rank, direct_dispatch=direct, split_batch=0 if mode == "none" else 1) for _ in range(S)]
        gr = grs[0]
        for q in grs:
            q.set_input(x)
            q.upload()                               # inputs resident in HBM before the timed region
            q.sync()
        exts = [torch.cuda.ExternalStream(q.stream(), device=torch.device("cuda", local_rank)) for q in grs]
        # EVERY graph output is gathered (YOLOv3-tiny: two heads = 215 475 B/image; mssd: loc + conf): the outputs of one
        # step are packed into one slot (each padded to the largest shard, so ragged --global-batch shards gather with one
        # equal-sized collective) and all-gathered with a single call
        n_out = gr.output_num()
        views, out_sizes = [], []
        for q in grs:
            vq = []
            for oi in range(n_out):
                out_ptr, out_bytes = q.output_device(oi)
                vq.append(torch.as_tensor(_CAI(out_ptr, out_bytes), device="cuda"))
            views.append(vq)
            out_sizes = [int(v.numel()) for v in vq]
        per_image = [b // args.batch for b in out_sizes]
        slot_off, slot_bytes = [], 0
        for b in per_image:
            slot_off.append(slot_bytes)
            slot_bytes += b * max_shard
        slots, gathered, works, slot_done, stalls, copied = None, None, {}, {}, [0], {}
        sides = [torch.cuda.Stream(device=torch.device("cuda", local_rank)) for _ in range(S)] if mode == "every" else None
        if mode != "none":
            slots = [[torch.zeros(slot_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)] for _ in range(S)]
            gathered = [[torch.empty(slot_bytes * world, dtype=torch.uint8, device="cuda") for _ in range(2)] for _ in range(S)]

        def gather(i, s_):
            for oi in range(n_out):
                slots[i][s_][slot_off[oi]:slot_off[oi] + out_sizes[oi]].copy_(views[i][oi], non_blocking=True)
            if direct and mode == "every":               # the staging buffers are free again once this event has fired
                copied[i] = copied.get(i) or torch.cuda.Event()
                copied[i].record()
            works[(i, s_)] = dist.all_gather_into_tensor(gathered[i][s_], slots[i][s_], async_op=True)

        def step(k):
            i = k % S
            if direct and mode == "every":
                # direct dispatch: nothing orders the pass against the side stream but the host.  The previous step's copy out of
                # the output staging buffers must be complete before this pass may overwrite them; the pass is awaited on its
                # queue's signal; copy + collective then run on the side stream while the next pass computes
                if copied.get(i) is not None:
                    copied[i].synchronize()
                grs[i].launch()
                grs[i].sync()
                s_ = (k // S) & 1
                with torch.cuda.stream(sides[i]):
                    if works.get((i, s_)) is not None:
                        ev = slot_done.get((i, s_))
                        if ev is not None and not ev.query():
                            stalls[0] += 1
                            ev.synchronize()
                        works[(i, s_)].wait()
                    gather(i, s_)
                    works[(i, s_)].wait()
                    ev = slot_done.setdefault((i, s_), torch.cuda.Event())
                    ev.record()
                return
            grs[i].launch()
            if mode == "every":
                s_ = (k // S) & 1
                with torch.cuda.stream(exts[i]):
                    if works.get((i, s_)) is not None:
                        # the slot's previous gather (two steps ago) must be complete before the slot is refilled: the HOST waits
                        # here when it is not -- at most two gathers are ever outstanding, the compute queue cannot run away from
                        # the collectives, and every such wait is counted (`gather_stalls` in the line)
                        ev = slot_done.get((i, s_))
                        if ev is not None and not ev.query():
                            stalls[0] += 1
                            ev.synchronize()
                        works[(i, s_)].wait()
                    gather(i, s_)
                # the slot's completion event, recorded behind the collective on a SIDE stream: the graph's own stream must not
                # wait for this step's gather (it overlaps the next step)
                with torch.cuda.stream(sides[i]):
                    works[(i, s_)].wait()
                    ev = slot_done.setdefault((i, s_), torch.cuda.Event())
                    ev.record()

        def drain():
            if mode == "final":                          # the last step's outputs of every stream, one collective each
                for q in grs:
                    q.sync()                             # direct dispatch: the passes are not on the stream the copies run on
                for i in range(S):
                    with torch.cuda.stream(exts[i]):
                        gather(i, 0)
            for (i, s_), w in works.items():
                if w is not None:
                    with torch.cuda.stream(sides[i] if (direct and mode == "every") else exts[i]):
                        w.wait()
            for q in grs:
                q.sync()
            torch.cuda.synchronize()

        for k in range(args.warmup):
            step(k)
        drain()

        def timed():
            """exactly K steps, barrier + synchronize on both sides, MAX over ranks"""
            if use_dist:
                dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(args.steps):
                step(k)
            drain()
            if use_dist:
                dist.barrier()
            torch.cuda.synchronize()
            e = time.perf_counter() - t0
            if use_dist:
                t = torch.tensor([e], dtype=torch.float64, device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                e = float(t.item())
            return e

        # --full: the region is repeated until the regions add up to --min-seconds (every rank derives the same count from the first
        # region's MAX-reduced time); the line carries the MEDIAN region
        els = [timed()]
        if args.full:
            for _ in range(repeats_for(els[0], args.min_seconds, args.max_repeats) - 1):
                els.append(timed())
        els.sort()
        el_ = els[len(els) // 2]
        info = {"el": el_, "el_min": els[0], "el_max": els[-1], "repeats": len(els),
                "n_out": n_out, "per_image": per_image, "out_sizes": out_sizes, "direct_packets": gr.direct_packets(), "mode": mode,
                "gather_stalls": stalls[0]}
        if keep:
            return info, grs
        for q in grs:
            q.close()
        return info, None

    # Which regions: N = 1 -> one region, no collective.  N > 1 -> BOTH gather modes, each in its own timed region of exactly K
    # steps: `every` first (the judged `value`: SURVEY 8(e) defines a per-batch gather overlapped with the next batch), then
    # `final` (side object: the images are independent, so a serving loop that keeps results on their rank pays one collective at
    # the end).  --gather final|every restricts the line to that one mode; a plain run (no --full) times `every` alone.
    side = {}
    if not use_dist:
        main_info, grs = region("none", args.direct, keep=True)
    elif args.gather == "both" and args.full:
        main_info, _ = region("every", args.direct)
        # the same K steps on the SAME dispatch path without any collective: what the N GPUs do when nothing is gathered -- the
        # like-for-like reference of `value` inside this very job (N x the N = 1 line's `value` on the direct path)
        rep_info, _ = region("none", args.direct)
        side["no_collective"] = {"value": total_images * args.steps / rep_info["el"], "ms_per_step": 1e3 * rep_info["el"] / args.steps,
                                 "what": "K steps on every rank on the same dispatch path (%s), no collective and no per-step wait: value / this = what the "
                                         "per-step gather costs (the host's wait for each pass included); compare with n_gpus x the N = 1 line's %s"
                                         % ("direct AQL dispatch" if rep_info["direct_packets"] else "hipGraph replay",
                                            "value" if rep_info["direct_packets"] else "hipgraph_replay.value")}
        fin_info, grs = region("final", args.direct, keep=True)
        side["gather_final"] = {"value": total_images * args.steps / fin_info["el"], "ms_per_step": 1e3 * fin_info["el"] / args.steps,
                                "what": "same K steps, no per-step collective (direct AQL dispatch, %d packets per step): every output of the LAST step "
                                        "all-gathered once, inside the timed region" % fin_info["direct_packets"]}
    else:
        main_info, grs = region("every" if args.gather == "both" else args.gather, args.direct, keep=True)
    gr = grs[0]
    # what the timed path computed in its last step (every stream's graph runs the same input)
    outs_all = grs[(args.steps - 1) % S].download() if rank == 0 and (args.full or args.dump_outputs) else None
    if rank == 0 and args.dump_outputs:
        dump_outputs(outs_all, args.dump_outputs)
    el = main_info["el"]
    n_out, per_image, out_sizes = main_info["n_out"], main_info["per_image"], main_info["out_sizes"]
    gather_mode = main_info["mode"]
    # the N > 1 `every` region replays hipGraphs (stream order); its N = 1 counterpart on the SAME dispatch path, so that a
    # scaling curve can be read against like for like: K more steps as hipGraph replays, reported as a side object
    if args.full and not use_dist and S == 1 and args.direct and rank == 0:
        rep_info, _ = region("none", 0)
        side["hipgraph_replay"] = {"value": total_images * args.steps / rep_info["el"], "ms_per_step": 1e3 * rep_info["el"] / args.steps,
                                   "what": "the same K steps as hipGraph replays on the graph's HIP stream -- the dispatch path of the N > 1 per-step-gather region"}

    # ---- the SURVEY §8(d) metric as tm_benchmark times it (tm_benchmark.cc:118-129): host buffer in -> H2D -> graph
    # -> D2H -> host buffer out, one blocking run after the other; reported beside `value`, never as `value` ----------
    host_to_host = None
    if args.full and rank == 0 and not use_dist:
        # SURVEY 8(d) asks for >= 50 timed iterations; a short --steps must not shrink this sample (the driver's K = 20 gave a
        # 1 ms region in round 2): at least 200 runs AND at least ~50 ms
        n_h2h = max(200, min(args.steps, 2000))
        gr.run_noreturn()
        t_probe = time.perf_counter()
        gr.run_noreturn()
        t_probe = time.perf_counter() - t_probe
        n_h2h = min(5000, max(n_h2h, int(0.05 / max(t_probe, 1e-6))))
        gr.run_noreturn()
        ts = []
        for _ in range(n_h2h):
            t1 = time.perf_counter()
            gr.run_noreturn()
            ts.append(time.perf_counter() - t1)
        ts.sort()
        in_bytes = int(np.asarray(x).nbytes)
        # the same loop with tamd_graph_run_async / tamd_graph_wait (interface.async_run / async_wait), two runs in flight
        outs2 = [gr.output_like(), gr.output_like()]
        gr.run_async(outs2[0])
        tp = time.perf_counter()
        for k in range(n_h2h):
            gr.run_async(outs2[(k + 1) & 1])
            gr.wait()
        gr.wait()
        tp = time.perf_counter() - tp
        gr.bind_default_outputs()
        host_to_host = {"pipelined_images_per_s": args.batch * n_h2h / tp,
                        "images_per_s_min": args.batch / ts[0], "images_per_s_median": args.batch / ts[len(ts) // 2],
                        "ms_min": 1e3 * ts[0], "ms_median": 1e3 * ts[len(ts) // 2], "runs": n_h2h,
                        "what": "tamd_graph_run(): memcpy into the pinned input (%d B) + ONE %s (upload kernel, launch list, download "
                                "kernel: %d B) + wait + copy out, blocking, 1 stream -- what tm_benchmark times; pipelined = "
                                "tamd_graph_run_async / tamd_graph_wait with two runs in flight (%s)"
                                % (in_bytes, "direct AQL pass on the graph's HSA queue" if gr.direct_packets() else "hipGraph", sum(out_sizes),
                                   "each run one burst on the same HSA queue, the second queued behind the first's closing packet"
                                   if gr.direct_packets() else "hipGraph on the stream")}

    # ---- roofline of the dominant kernel (HIP events on the launch stream, same process) -----------
    roofline = None
    if args.full and rank == 0:
        roofline = roofline_of(gr, args.model, args.dtype, args.batch, args.u8_integer, el / args.steps)

    # ---- the other BASELINE configurations, each on its shipped plan, in this same process (N = 1) ----------
    configs = None
    if args.full and rank == 0 and not use_dist and S == 1 and args.configs != "none" and \
            (args.configs == "all" or (args.model, args.dtype, args.batch, args.u8_integer) == ("mobilenet_v1", "int8", 1, False)):
        configs = {}
        for name, dtype, batch, what in SIDE_CONFIGS:
            if (name, dtype, batch) == (args.model, args.dtype, args.batch):
                continue
            try:
                configs["%s_%s_b%d" % (name, dtype, batch)] = side_config(name, dtype, batch, what, local_rank, args.direct)
            except Exception as e:       # noqa: BLE001 -- a side configuration must never take the judged line down with it
                configs["%s_%s_b%d" % (name, dtype, batch)] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        if plan_tmp:
            os.environ["TAMD_PLAN_CACHE"] = plan_tmp

    # ---- CPU baseline: the real reference backend on this host's cores (rank 0, N=1 only) ----------
    cpu = None
    if args.full and rank == 0 and (world == 1 and not args.force_dist) and not args.no_cpu_baseline:
        cpu = cpu_baseline(tm_bytes, g, x, args.batch, args.cpu_seconds, u8)

    head_sha = output_sha(outs_all) if (args.full and rank == 0) else None
    head_golden = golden_sha(args.model, args.dtype, args.batch) if (args.full and rank == 0 and not args.u8_integer) else None
    n_direct = main_info["direct_packets"]
    n_halves = gr.halves()
    prerun_ms = gr.prerun_ms()
    for q in grs:
        q.close()

    def flush_c_stdio():
        # librccl announces itself through C stdio ("Librccl path : ..."), which a pipe buffers until exit: every rank flushes it
        # BEFORE rank 0 prints, so that the JSON line is the last line of the job's stdout
        try:
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass

    if plan_tmp and os.path.exists(plan_tmp):
        os.remove(plan_tmp)
    flush_c_stdio()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
        flush_c_stdio()
    if rank == 0:
        value = total_images * args.steps / el
        line = {
            "metric": "images/sec int8 MobileNet-v1 224x224" if (args.model, args.dtype) == ("mobilenet_v1", "int8")
            else "images/sec %s %s%s" % (args.dtype, args.model, " (integer path, <= 1 LSB per layer)" if args.u8_integer else ""), "value": value, "unit": "images/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * el / args.steps, "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak", "vs_baseline": None, "dtype": ("int8 MFMA, int32 sums (uint8 integer path: within one step of the reference per layer, NOT byte-identical)" if args.u8_integer
                                                                                else "f32 (uint8 simulated in fp32, as the reference)") if u8 else "int8",
            "data": "synthetic",
            "config": {"workload": "%s %s batch=%d per GPU%s, weights = seeded synthetic tmfile, input resident in HBM, "
                                   "%s, %d stream(s)" % (args.model, args.dtype, args.batch,
                                                                      " (BASELINE configs[1])" if (args.model, args.dtype, args.batch) == ("mobilenet_v1", "int8", 1) else "",
                                                                      ("direct AQL dispatch of the launch list (%d packets per step)" % n_direct if n_direct else "hipGraph replay")
                                                                      + (", the batch as two device graphs of %d images side by side on their own queues behind one handle (tamd_options.split_batch)" % (args.batch // 2) if n_halves else ""), S),
                       "streams": S, "halves": n_halves,
                       "global_batch": total_images, "parallelism": "dp%d" % world,
                       "collectives": ("rccl broadcast(tmfile) once + one all_gather of all %d output(s) (%d B/image) %s"
                                       % (n_out, sum(per_image), "per step, overlapped with the next step" if gather_mode == "every"
                                          else "of the last step, inside the timed region (no per-step collective: independent images)"))
                       if use_dist else "none"},
            "timed_regions": {"repeats": main_info["repeats"], "steps_each": args.steps, "ms_per_step_min": 1e3 * main_info["el_min"] / args.steps,
                              "ms_per_step_max": 1e3 * main_info["el_max"] / args.steps,
                              "what": "the region of exactly K steps (barrier + synchronize on both sides, MAX over ranks) repeated until the regions "
                                      "add up to >= %g s; value / ms_per_step = the MEDIAN region" % args.min_seconds if args.full
                                      else "one region of exactly K steps (barrier + synchronize on both sides, MAX over ranks)"},
            "roofline": roofline, "configs": configs, "cpu_baseline": cpu, "host_to_host": host_to_host,
            # the two readings of the metric side by side.  `value` follows the bench contract of this build ("whole-job throughput with
            # inputs already resident in HBM when the timed region starts ... the PCIe-inclusive rate is never `value`"); SURVEY 8(d) /
            # tm_benchmark.cc:118-129 time the blocking host-to-host run_graph, which is `host_to_host_images_per_s` (median of
            # host_to_host.runs blocking runs) and, with two runs in flight, `host_to_host_pipelined_images_per_s`
            "value_definition": "device-resident: %d step(s) of the launch list with the input batch already in HBM, outputs left in HBM" % args.steps,
            "host_to_host_images_per_s": host_to_host["images_per_s_median"] if host_to_host else None,
            "host_to_host_pipelined_images_per_s": host_to_host["pipelined_images_per_s"] if host_to_host else None,
            "prerun_ms": prerun_ms, "shipped_plan": shipped_plan,
            # which N = 1 figure a scaling curve of `value` has to be read against: the N = 1 line's `value` when both are direct AQL
            # dispatch (round 5: the per-step-gather region no longer needs the hipGraph replay), else its `hipgraph_replay`
            "scaling_baseline_key": "value" if n_direct else "hipgraph_replay",
            "gather_stalls": main_info.get("gather_stalls", 0) if use_dist else None,
            **side,
            "output_checksum": int(np.asarray(outs_all[0], dtype=np.int64).sum()) if head_sha else None,
            # every output of the last step against the REAL reference's result on the same seeded input (tests/golden/bench_outputs_sha256.json)
            "output_sha256": head_sha, "golden_sha256": head_golden, "golden_match": (head_sha == head_golden) if head_golden else None,
        }
        if cpu:
            line["speedup_vs_cpu_reference"] = value / cpu["value"] if cpu["value"] else None
        print(json.dumps(line), flush=True)


# the BASELINE configurations beside the headline (configs[1] = mobilenet_v1 int8 b1): per-GPU shards of configs[3] / configs[4]
SIDE_CONFIGS = [("mobilenet_v1", "int8", 1, "BASELINE configs[1]"),
                ("mobilenet_v1", "int8", 64, "configs[1]'s model at batch 64 (throughput line)"),
                ("resnet50", "int8", 32, "BASELINE configs[2]"),
                ("yolov3_tiny", "uint8", 8, "BASELINE configs[3]: batch 64 over 8 GPUs = 8 per GPU, byte-exact path"),
                ("mssd", "uint8", 16, "BASELINE configs[4]: batch 128 over 8 GPUs = 16 per GPU (mssd = the reference's MobileNet-SSD), byte-exact path")]
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "bench_outputs_sha256.json")


def dump_outputs(outs, out_dir, limit_bytes=64_000_000):
    """every output array as out_dir/output<i>.npy in float32 (float64 stays float64).  A set larger than limit_bytes keeps, of each
    output, a fixed seeded sample of its flattened elements (in index order) in proportion to its size."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrs = [np.asarray(o, np.float64 if o.dtype == np.float64 else np.float32) for o in outs]
    total = sum(a.nbytes for a in arrs)
    for i, a in enumerate(arrs):
        if total > limit_bytes:
            keep = a.size * limit_bytes // total
            a = a.reshape(-1)[np.sort(np.random.default_rng(i).choice(a.size, keep, replace=False))]
        np.save(os.path.join(out_dir, "output%d.npy" % i), a)


def repeats_for(first_region_s, min_seconds, max_repeats):
    """how many regions of K steps make up >= min_seconds, given what the first one took (>= 1, <= max_repeats)"""
    if first_region_s <= 0:
        return max(1, max_repeats)
    n = int(-(-min_seconds // first_region_s))
    return max(1, min(int(max_repeats), n))


def roofline_of(gr, model, dtype, batch, u8_integer, step_s):
    """dominant kernel family of the graph's launch list: algorithmic bytes (or MACs) / average launch duration measured with HIP events
    (tamd_graph_profile), against the HBM / dense MFMA peak; `traffic` from the committed PMC summary of this workload"""
    u8 = dtype == "uint8"
    prof = gr.profile(20)
    fam = {}
    for k in prof:
        # family = the kernel's base name: template variants (tile shapes, K splits) of one kernel count together
        f = fam.setdefault(kernel_family(k["kernel"]), {"ms": 0.0, "bytes": 0.0, "macs": 0.0, "launches": 0})
        f["ms"] += k["ms"]; f["bytes"] += k["bytes"]; f["macs"] += k["macs"]; f["launches"] += 1
    dom = max(fam, key=lambda n: fam[n]["ms"])
    d = fam[dom]
    t_hbm = d["bytes"] / (HBM_PEAK_GBS * 1e9)
    mfma_peak = MFMA_F32_PEAK_TOPS if (u8 and not u8_integer) else MFMA_I8_PEAK_TOPS
    t_mfma = 2.0 * d["macs"] / (mfma_peak * 1e12)
    if t_hbm >= t_mfma:
        ach = d["bytes"] / (d["ms"] * 1e-3) / 1e9
        roofline = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS}
    else:
        ach = 2.0 * d["macs"] / (d["ms"] * 1e-3) / 1e12
        roofline = {"bound": "mfma", "achieved": ach, "peak": mfma_peak, "unit": "TOP/s", "frac": ach / mfma_peak}
    sum_ms = max(sum(f["ms"] for f in fam.values()), 1e-12)
    roofline.update({"kernel": dom, "launches_per_step": d["launches"], "avg_launch_us": 1e3 * d["ms"] / d["launches"],
                     # (a graph compiled as two half-batch device graphs launches half-batch kernels: their PMC pass is the half batch's)
                     "traffic": pmc_traffic(model, dtype + ("_int" if u8_integer else ""), batch // 2 if gr.halves() else batch, dom),
                     "algorithmic_bytes_per_launch": d["bytes"] / d["launches"],
                     "algorithmic_macs_per_launch": d["macs"] / d["launches"],
                     # whole-step matrix-core utilisation (BASELINE metric's second half): all MACs of the step
                     # over the summed kernel time, against the dense MFMA peak of the compute dtype
                     "mfma_util_pct": 100.0 * 2.0 * sum(f["macs"] for f in fam.values()) / (sum_ms * 1e-3) / (mfma_peak * 1e12),
                     "kernel_time_share": d["ms"] / sum_ms,
                     "sum_kernel_ms_per_step": sum(f["ms"] for f in fam.values()),
                     # SURVEY 8(d)'s per-layer roofline of the WHOLE step: sum over launches of max(2 MAC / P, bytes / BW), against the step's clock
                     "step_roofline_us": 1e6 * sum(max(2.0 * k["macs"] / (mfma_peak * 1e12), k["bytes"] / (HBM_PEAK_GBS * 1e9)) for k in prof),
                     "step_frac": sum(max(2.0 * k["macs"] / (mfma_peak * 1e12), k["bytes"] / (HBM_PEAK_GBS * 1e9)) for k in prof) / max(step_s, 1e-12),
                     "launch_durations": "HIP events around eager back-to-back launches of each kernel on the graph's stream "
                                         "(tamd_graph_profile) -- the figure rocprofv3 --kernel-trace agrees with"})
    if gr.direct_packets():
        # the timed loop dispatched the same launches as AQL packets with cheaper boundaries (csrc/direct.cc): HIP events do not see
        # that queue.  Round 6: the HSA runtime's own dispatch profiling does (tamd_graph_direct_timestamps: start / end stamp of every
        # packet of back-to-back direct passes, no tool in the process) -- the dominant family's launch duration ON THE TIMED PATH
        try:
            rows = gr.direct_timestamps(100 if step_s < 2e-4 else 30)
            famrows = [r for r in rows if symbol_in_family(r[0], dom)]
            if famrows:
                us = sum(r[1] for r in famrows) / len(famrows)
                per = (d["bytes"] / d["launches"]) / 1e9 / HBM_PEAK_GBS if t_hbm >= t_mfma else (2.0 * d["macs"] / d["launches"]) / 1e12 / mfma_peak
                roofline["hsa_dispatch_stamps"] = {
                    "avg_launch_us": us, "launches_matched": len(famrows), "frac": per / (us * 1e-6),
                    "avg_gap_to_next_packet_us": sum(r[2] for r in rows) / len(rows),
                    "sum_durations_us_per_pass": sum(r[1] for r in rows), "sum_gaps_us_per_pass": sum(r[2] for r in rows),
                    "what": "direct AQL passes with every packet stamped by hsa_amd_profiling_get_dispatch_time (the timestamps a kernel trace "
                            "reports, read without a tool): mean duration of the dominant family's packets on the path the timed loop runs, "
                            "and the device-side gap between consecutive packets"}
        except Exception as e:       # noqa: BLE001 -- a measurement extra must never take the line down
            roofline["hsa_dispatch_stamps"] = {"error": str(e)[:200]}
        # The step's own clock bounds what a launch of the dominant family cost there: its share of the step
        est_us = 1e3 * (d["ms"] / sum_ms) * (step_s * 1e3) / d["launches"]
        roofline["direct_dispatch"] = {
            "avg_launch_us_from_step_clock": est_us,
            "frac_from_step_clock": (d["bytes"] / d["launches"]) / (est_us * 1e-6) / 1e9 / HBM_PEAK_GBS if t_hbm >= t_mfma
            else (2.0 * d["macs"] / d["launches"]) / (est_us * 1e-6) / 1e12 / mfma_peak,
            "what": "timed loop = direct AQL dispatch: ms_per_step x the family's share of the summed HIP-event durations / its launches; "
                    "`frac` above stays the HIP-event figure (conservative: it carries HIP's launch boundary)"}
    return roofline


def golden_sha(model, dtype, batch):
    """sha256 of every output of this configuration as the REAL reference computes it on bench.py's rank-0 input (seed 1000):
    tests/golden/bench_outputs_sha256.json, written by tests/golden/make_bench_sha.py; None when the file does not hold it"""
    try:
        e = json.load(open(GOLDEN_SHA)).get("%s_%s_b%d" % (model, dtype, batch))
        return [o["sha256"] for o in e["outputs"]] if e else None
    except (OSError, ValueError, KeyError):
        return None


def output_sha(outs):
    import hashlib

    import numpy as np
    return [hashlib.sha256(np.ascontiguousarray(o).tobytes()).hexdigest() for o in outs]


def side_config(model, dtype, batch, what, gpu_index, direct, steps=100, regions=3, warmup=10):
    """One BASELINE configuration beside the headline, timed in this process: its own graph on its shipped plan, input resident in HBM,
    `regions` regions of `steps` passes each (synchronised on both sides), the MEDIAN region reported; roofline of its dominant
    kernel family; sha256 of its outputs against the real reference's (golden).  No CPU baseline, no host-to-host loop."""
    import tempfile

    from tengine_amd import capi, models, plans, tm2
    u8 = dtype == "uint8"
    plan = os.path.join(tempfile.gettempdir(), "tamd_plan_%d_%s_%s_b%d.txt" % (os.getpid(), model, dtype, batch))
    shipped = plans.seed(plan, model, dtype, batch)
    os.environ["TAMD_PLAN_CACHE"] = plan          # (the library re-reads its table when the path changes: csrc/plan_cache.hip)
    gr = None
    try:
        g = models.build(model, dtype, batch)
        tm_bytes = tm2.write_tm2(g)
        x = models.synth_input(g, 1000, tm2.DT_UINT8 if u8 else tm2.DT_INT8)
        gr = capi.Graph(tm_bytes, batch=batch, gpu_index=gpu_index, direct_dispatch=bool(direct))
        gr.set_input(x)
        gr.upload()
        gr.sync()
        prerun_ms = gr.prerun_ms()
        for _ in range(warmup):
            gr.launch()
        gr.sync()
        els = []
        for _ in range(regions):
            t0 = time.perf_counter()
            for _ in range(steps):
                gr.launch()
            gr.sync()
            els.append(time.perf_counter() - t0)
        els.sort()
        el = els[len(els) // 2]
        outs = gr.download()
        sha, want = output_sha(outs), golden_sha(model, dtype, batch)
        r = roofline_of(gr, model, dtype, batch, False, el / steps)
        dispatch = "direct AQL dispatch (%d packets per step)" % gr.direct_packets() if gr.direct_packets() else "hipGraph replay"
        halves = gr.halves()
        if halves:
            dispatch += ", as two device graphs of batch %d side by side on their own queues behind one handle (tamd_options.split_batch)" % (batch // 2)
        gr.close()
        gr = None
        try:
            other = other_form(tm_bytes, model, dtype, batch, x, gpu_index, direct, steps, regions, warmup, want, 1 if halves else 2)
            if not halves and not other["halves"]:     # (YOLOv3-tiny's Upsample, the SSD heads: not in the batch-wise independent operator list)
                other = {"halves": 0, "what": "this graph cannot be halved (operators outside the batch-wise independent list): one launch list is its only form"}
        except Exception as e:                     # a side measurement of a side configuration: never at the cost of the line
            other = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        return {"what": what, "ms_per_step": 1e3 * el / steps, "images_per_s": batch * steps / el, "halves": halves,
                ("one_launch_list" if halves else "two_half_batches"): other,
                "ms_per_step_min": 1e3 * els[0] / steps, "ms_per_step_max": 1e3 * els[-1] / steps, "steps": steps * regions, "regions": regions,
                "dispatch": dispatch,
                "roofline": {k: r[k] for k in ("bound", "kernel", "frac", "achieved", "peak", "unit", "traffic", "algorithmic_bytes_per_launch",
                                               "algorithmic_macs_per_launch", "avg_launch_us", "launches_per_step", "mfma_util_pct",
                                               "step_roofline_us", "step_frac")},
                "output_sha256": sha, "golden_sha256": want, "golden_match": (sha == want) if want else None,
                "prerun_ms": prerun_ms, "shipped_plan": shipped}
    finally:
        if gr is not None:
            gr.close()
        if os.path.exists(plan):
            os.remove(plan)


def other_form(tm_bytes, model, dtype, batch, x, gpu_index, direct, steps, regions, warmup, want, split_batch):
    """The same configuration in the OTHER form the library has for a batch -- one launch list (split_batch = 1) when the configuration's
    own graph took the two-half-batch form, two half-batch graphs side by side (split_batch = 2) when it did not -- through the same
    single handle, same images, same region protocol, outputs against the same golden.  A SIDE figure: it shows inside the driver's own
    run what the form costs or buys; `ms_per_step` / `images_per_s` of the configuration are its default form's."""
    from tengine_amd import capi
    gr = capi.Graph(tm_bytes, batch=batch, gpu_index=gpu_index, direct_dispatch=bool(direct), split_batch=split_batch)
    try:
        gr.set_input(x)
        gr.upload()
        gr.sync()
        for _ in range(warmup):
            gr.launch()
        gr.sync()
        els = []
        for _ in range(regions):
            t0 = time.perf_counter()
            for _ in range(steps):
                gr.launch()
            gr.sync()
            els.append(time.perf_counter() - t0)
        els.sort()
        el = els[len(els) // 2]
        sha = output_sha(gr.download())
        return {"what": "tamd_options.split_batch = %d: %s; same images, same %d x %d steps"
                        % (split_batch, "two device graphs of batch %d side by side on their own queues" % (batch // 2) if gr.halves() else "one launch list", regions, steps),
                "halves": gr.halves(), "ms_per_step": 1e3 * el / steps, "images_per_s": batch * steps / el, "ms_per_step_min": 1e3 * els[0] / steps,
                "ms_per_step_max": 1e3 * els[-1] / steps, "golden_match": (sha == want) if want else None}
    finally:
        gr.close()


def kernel_family(step_kernel):
    """the family a launch is booked under in `roofline`: the step's kernel name without its template / fusion suffixes and
    without the tile shape -- conv_u8_patch_32x64<3x3>+relu -> conv_u8_patch, conv_u8_mfma_64x64k64+relu+maxpool -> conv_u8_mfma,
    pwdw_i8<s1,7x14,512> -> pwdw_i8"""
    return re.sub(r"_\d+x\d+(x\d+)?(k\d+)?$", "", step_kernel.split("<")[0].split("+")[0])


def symbol_in_family(name, family):
    """does the kernel SYMBOL `name` (rocprofv3 / HSA packet name) belong to the step family `family` (kernel_family of a step name)?"""
    # the pwdw_i8_kernel<STEPS, MODE, CHUNKED, PROD[, WIN]> template serves four step families: tell them apart by MODE / PROD
    m = re.search(r"pwdw_i8(?:_coh)?_kernel<\s*\d+,\s*(\d+),\s*\w+,\s*(\d+)(?:,\s*\d+)*>", name)
    if m:
        mode, prod = int(m.group(1)), int(m.group(2))
        fam = "firstdw_i8" if prod == 1 else "pwpool_i8" if mode == 0 else "pw_small_i8" if mode == 4 else "pwdw_i8"
        return fam == family
    # step names vs kernel symbols where they differ
    alias = {"conv_u8_mfma": "conv_u8_gemm_k", "conv_u8_patch": "conv_u8_patch_k", "conv_pgemm_i8": "conv_pgemm", "conv_igemm_i8": "conv_igemm",
             "conv_u8i": "conv_u8i_k"}
    return alias.get(family, family) in name


def pmc_traffic(model, dtype, batch, family):
    """HBM bytes per launch of the dominant kernel family, from the committed rocprofv3 PMC summary of this workload
    (profiles/rNN_traffic_<model>_<dtype>_b<batch>.json, the newest round's: separate --pmc FETCH_SIZE / WRITE_SIZE passes, scaled by the
    same-session streaming-copy calibration -- tools/collect_profiles.sh, tools/traffic_summary.py); None when this
    workload has no PMC pass (counters cannot be collected from inside the timed process)."""
    import glob
    found = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_traffic_%s_%s_b%d.json" % (model, dtype, batch)))
                   + glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9][a-z]_traffic_%s_%s_b%d.json" % (model, dtype, batch))))      # (a second pass of a round: r05b_)
    if not found:
        return None
    path = found[-1]
    ks = json.load(open(path))["kernels"]
    tot, n = 0.0, 0

    def member(name):
        return symbol_in_family(name, family)

    for name, v in ks.items():
        if member(name) and v["hbm_read_bytes_per_launch"] is not None:
            tot += (v["hbm_read_bytes_per_launch"] + (v["hbm_write_bytes_per_launch"] or 0.0)) * v["launches"]
            n += v["launches"]
    return tot / n if n else None


def cpu_baseline(tm_bytes, g, x, batch, budget_s, u8=False):
    """Reference `source/device/cpu` path through create_graph/prerun/run_graph on the host cores, swept over thread
    counts {1, 8, 32, physical cores, logical cpus} (SURVEY §8d asks for {1, all physical cores}; 256 OpenMP threads on
    a 256-way SMT host oversubscribe the small batch-1 layers).  `value` = the BEST point of the sweep, `cores` = the
    threads of that point, the whole sweep is in `sample`."""
    import numpy as np
    logical = os.cpu_count() or 1
    physical = physical_cores() or logical
    # The reference takes omp_get_max_threads() as its core count the first time it is asked (source/system/cpu.c:110, cached),
    # caps it at 64 and builds the all-cores mask as ((size_t)1 << count) - 1 -- zero for 64, and then every kernel runs on one
    # thread whatever options.num_thread says (a flat sweep).  Asking OpenMP for fewer threads BEFORE the reference's first graph
    # (what OMP_NUM_THREADS=<n> in the environment does) keeps the mask valid with the sources untouched.  Default cap: the
    # smallest of the container's CPU allowance (cgroup cpu.max), the physical cores and 63; TAMD_BENCH_REF_THREADS=<n> pins it,
    # =0 switches the cap off (the reference as it probes this host by itself).
    cap, cap_why = ref_thread_cap(logical, physical)
    if cap < logical:
        try:
            ctypes.CDLL("libgomp.so.1").omp_set_num_threads(cap)
        except (OSError, AttributeError):
            cap, cap_why = logical, "libgomp not reachable: no cap"
    sweep = sorted({min(t, cap) for t in (1, 4, 8, 16, 32, physical, logical) if t >= 1})
    if len(sweep) > 5:
        sweep = sorted(set(sweep[:2] + sweep[-3:]))
    try:
        from oracle import ref_capi
        if not ref_capi.available():
            raise FileNotFoundError
        pts = []
        per_point = budget_s / len(sweep)
        for threads in sweep:
            rg = ref_capi.RefGraph(tm_bytes, ref_capi.MODE_UINT8 if u8 else ref_capi.MODE_INT8, threads)
            rg.set_input(x)
            t0 = time.perf_counter()
            rg.run()                                   # warm-up (weight packing, pool alloc)
            first = time.perf_counter() - t0
            ts, t_end = [], time.perf_counter() + per_point
            # bounded sample: a point whose single run already exceeds its share of the budget (large batches at 1 thread) is
            # timed once more and left at that
            while (time.perf_counter() < t_end or len(ts) < 3) and not (ts and first > per_point):
                t0 = time.perf_counter()
                rg.run()
                ts.append(time.perf_counter() - t0)
            rg.close()
            pts.append((threads, min(ts), float(np.mean(ts)), len(ts)))
        best = min(pts, key=lambda p: p[1])
        flat = max(p[1] for p in pts) < 1.08 * min(p[1] for p in pts) and len(pts) > 2
        note = "; OpenMP capped at %d threads before the reference's first graph (%s): works around source/system/cpu.c:110-121,269" % (cap, cap_why) if cap < logical else ""
        if flat and logical >= 64:
            # source/system/cpu.c:120-121,269: core_count is capped at 64 and the all-cores mask is ((size_t)1 << core_count) - 1,
            # which is 0 on x86-64 for 64 -> get_cpu_mask_count() = 0 -> num_thread = 0: on a >= 64-CPU host the reference
            # runs its kernels single-threaded whatever options.num_thread says (the sweep is flat)
            note += ("; the sweep is flat because the reference's own CPU probing (source/system/cpu.c:120-121,269) yields a zero core "
                    "mask on a host with >= 64 logical CPUs and its kernels run single-threaded here")
        out = {"value": batch / best[1], "unit": "images/s", "cores": 1 if (flat and logical >= 64) else best[0], "kind": "reference",
               "physical_cores": physical, "logical_cpus": logical, "cgroup_cpu_max": cgroup_cpu_max(), "openmp_cap": cap if cap < logical else None,
               "sweep": [{"threads": p[0], "min_ms": 1e3 * p[1], "mean_ms": 1e3 * p[2], "runs": p[3]} for p in pts],
               "sample": "timed run_graph() calls of the same tmfile/input (batch %d) at each requested thread count of the sweep (%s), "
                         "%.0f s of CPU work in total; value = best point (min %.1f ms); reference CPU backend built -O3 -mfma "
                         "-fopenmp from the unmodified sources%s"
                         % (batch, ", ".join("%d thr: %.1f ms" % (p[0], 1e3 * p[1]) for p in pts), budget_s, 1e3 * best[1], note)}
        # second opinion where the reference cannot use the cores: the C restatement (oracle/tg_oracle.c, OpenMP over all
        # available cores) on the same input -- kind "port", reported beside the reference figure, never instead of it
        try:
            from oracle import oracle
            nthr = min(32, logical)
            cm = cgroup_cpu_max()
            if cm and cm.split()[0].isdigit():          # "quota period": the container's CPU allowance
                nthr = max(1, min(nthr, int(cm.split()[0]) // max(1, int(cm.split()[1]))))
            try:
                ctypes.CDLL("libgomp.so.1").omp_set_num_threads(nthr)
            except OSError:
                pass
            oracle.run_graph(g, x)
            ts, t_end = [], time.perf_counter() + min(4.0, budget_s / 3)
            while time.perf_counter() < t_end or len(ts) < 2:
                t0 = time.perf_counter()
                oracle.run_graph(g, x)
                ts.append(time.perf_counter() - t0)
            out["port_openmp"] = {"value": batch / min(ts), "unit": "images/s", "min_ms": 1e3 * min(ts), "runs": len(ts),
                                  "kind": "port", "threads": nthr,
                                  "what": "oracle/tg_oracle.c restatement (plain C, OpenMP) on the container's CPU allowance"}
        except Exception as e:       # noqa: BLE001 -- the port is optional evidence
            out["port_openmp"] = {"error": str(e)[:200]}
        return out
    except (FileNotFoundError, OSError):
        from oracle import oracle
        oracle.run_graph(g, x)
        ts, t_end = [], time.perf_counter() + budget_s
        while time.perf_counter() < t_end or len(ts) < 3:
            t0 = time.perf_counter()
            oracle.run_graph(g, x)
            ts.append(time.perf_counter() - t0)
        return {"value": batch / min(ts), "unit": "images/s", "cores": logical, "kind": "port",
                "sample": "%d timed oracle passes (batch %d), min %.1f ms" % (len(ts), batch, 1e3 * min(ts))}


def cgroup_cpus():
    """whole CPUs of the container's cgroup allowance ("quota period" in cpu.max), None when unlimited / unreadable"""
    cm = cgroup_cpu_max()
    if cm:
        f = cm.split()
        if len(f) == 2 and f[0].isdigit() and f[1].isdigit() and int(f[1]) > 0:
            return max(1, -(-int(f[0]) // int(f[1])))
    return None


def ref_thread_cap(logical, physical, env=None):
    """(threads OpenMP is limited to before the reference library's first graph, why).  See cpu_baseline."""
    env = os.environ.get("TAMD_BENCH_REF_THREADS") if env is None else env
    if env is not None and env.strip().isdigit():
        n = int(env)
        if n == 0:
            return logical, "TAMD_BENCH_REF_THREADS=0: no cap"
        return max(1, min(n, 63, logical)), "TAMD_BENCH_REF_THREADS"
    allow = cgroup_cpus()
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = logical
    cands = [("cgroup cpu.max allowance", allow), ("physical cores", physical), ("scheduler affinity", aff), ("the reference's 63-core limit", 63)]
    why, cap = min(((w, c) for w, c in cands if c), key=lambda e: e[1])
    return max(1, min(cap, logical)), why


def cgroup_cpu_max():
    try:
        return open("/sys/fs/cgroup/cpu.max").read().strip()
    except OSError:
        return None


def physical_cores():
    """distinct (package, core) pairs of /proc/cpuinfo; None when it cannot be read"""
    try:
        cores, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
        return len(cores) or None
    except OSError:
        return None


def respawn(args):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU.  Fails
    (rc != 0) when the node cannot host N ranks -- never a silent N=1 line."""
    import socket
    import subprocess
    if not args.dry_run:
        import torch
        have = torch.cuda.device_count()
        if have < args.gpus:
            raise SystemExit("bench.py: --gpus %d but only %d HIP device(s) visible" % (args.gpus, have))
    port = args.master_port
    if not port:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    rc = subprocess.call(cmd, env=env)
    if rc != 0:
        raise SystemExit(rc)


def dry_run(args, rank, world):
    """CPU/gloo check of the N-rank plumbing (no device, no compute): tmfile broadcast + integrity check, native-format
    reload on every rank, shard_range over --global-batch (or --batch per rank), ONE all_gather of every graph output
    padded to the largest shard, trimmed back to the global image order.  The outputs are rank/image tagged bytes, not
    results; the line says dry_run and carries value null so it can never be read as a measurement."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from tengine_amd import dist as tdist
    from tengine_amd import models, tm2
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        total = args.global_batch if args.global_batch else world * args.batch
        start, count = tdist.shard_range(total, world, rank)
        counts = [tdist.shard_range(total, world, r)[1] for r in range(world)]
        tm_bytes = None
        if rank == 0:
            tm_bytes = tm2.write_tm2(models.build(args.model, args.dtype, 1))
        tm_bytes = tdist.broadcast_tmfile(tm_bytes, dist, "cpu")
        g = tm2.read_tm2(tm_bytes)
        outs = [g.tensors[g.nodes[ni].outputs[0]] for ni in g.output_nodes]
        per_image = [int(np.prod(t.dims[1:])) for t in outs]
        ok = True
        for k in range(max(1, min(args.steps, 3))):
            gathered = []
            for oi, b in enumerate(per_image):
                local = torch.empty((count, b), dtype=torch.uint8)
                for j in range(count):
                    local[j] = (start + j + 7 * oi + k) % 251           # tag: global image index
                gathered.append(tdist.all_gather_outputs(local, dist, counts))
            for oi, gt in enumerate(gathered):
                want = (torch.arange(total) + 7 * oi + k) % 251
                ok = ok and gt.shape == (total, per_image[oi]) and bool((gt[:, 0].long() == want).all()) and bool((gt[:, -1].long() == want).all())
        flag = torch.tensor([1 if ok else 0])
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) != 1:
            raise SystemExit("bench.py --dry-run: gathered outputs are not in global image order")
        if rank == 0:
            multi = world > 1
            print(json.dumps({"metric": "images/sec %s %s" % (args.dtype, args.model), "value": None, "unit": "images/s",
                              "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "dry_run": True,
                              "scaling": "strong" if args.global_batch else "weak",
                              # the keys a measured N > 1 line carries (null here: nothing was measured)
                              "scaling_baseline_key": "value" if args.direct else "hipgraph_replay", "gather_stalls": None,
                              "gather_final": {"value": None} if multi and args.gather == "both" else None,
                              "no_collective": {"value": None} if multi and args.gather == "both" else None,
                              "config": {"workload": "%s %s: gloo plumbing check only, no device work" % (args.model, args.dtype),
                                         "global_batch": total, "shards": counts, "outputs": len(per_image),
                                         "gather_bytes_per_image": sum(per_image), "tmfile_bytes": len(tm_bytes),
                                         "parallelism": "dp%d" % world}}))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
