"""Direct dispatch (tamd_options.direct_dispatch, csrc/direct.cc): tamd_graph_launch replays the recorded launch list as AQL
packets on the graph's own HSA queue.  Same kernels, same arguments, same bytes as the hipGraph replay -- checked against the
oracle and against the hipGraph path for an int8, a uint8 and an fp32 model (single-struct and multi-scalar argument lists,
dynamic LDS, 1-D and 3-D grids), mixed with the stream-ordered entry points, and timed."""
import numpy as np
import pytest

from oracle import oracle
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
NP = {"int8": DT_INT8, "uint8": DT_UINT8, "fp32": DT_FP32}


def hip_runtime_of_the_library():
    """ctypes handle whose hipMemcpy is the one libtengine_amd.so itself calls (see the test below)"""
    import ctypes as C
    L = capi.lib()
    L.hipMemcpy.restype = C.c_int
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return L


def test_the_name_libamdhip64_is_not_the_librarys_runtime_once_torch_is_loaded():
    """the root cause of round 5's flake, pinned: after `import torch` behind the library, dlopen("libamdhip64.so") is another runtime
    (another hipMemcpy address) than the one the library's dependency tree holds -- tests must never read device memory through it"""
    import ctypes as C
    capi.lib()
    import torch  # noqa: F401
    mine = C.cast(hip_runtime_of_the_library().hipMemcpy, C.c_void_p).value
    maps = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
    if len(maps) > 1:                      # torch's bundled copy is mapped beside ROCm's
        other = C.cast(C.CDLL("libamdhip64.so").hipMemcpy, C.c_void_p).value
        assert other != mine
    back = np.zeros(64, np.uint8)
    g = models.build("mobilenet_v1", "int8", 1)
    gr = capi.Graph(tm2.write_tm2(g))
    p, n = gr.output_device(0)
    assert hip_runtime_of_the_library().hipMemcpy(back.ctypes.data, p, min(n, 64), 2) == 0
    gr.close()


def _resident(gr, x, launches):
    gr.set_input(x)
    gr.upload()
    for _ in range(launches):
        gr.launch()
    gr.sync()
    return gr.download()


@pytest.mark.parametrize("name,dtype,batch", [("mobilenet_v1", "int8", 1), ("mobilenet_v1", "int8", 8), ("resnet50", "int8", 2),
                                              ("yolov3_tiny", "uint8", 1), ("mssd", "uint8", 2), ("squeezenet_v1.1", "fp32", 1)])
def test_direct_dispatch_same_bytes_as_graph_replay(name, dtype, batch):
    g = models.build(name, dtype, batch, device_only=(name != "mobilenet_v1"))      # logits-only graphs (a softmaxed output is mostly zeros)
    x = models.synth_input(g, 77, NP[dtype])
    b = tm2.write_tm2(g)
    ref = capi.Graph(b)
    want = _resident(ref, x, 1)
    ref.close()
    gr = capi.Graph(b, direct_dispatch=True)
    assert gr.direct_packets() >= gr.kernel_num() > 0, "direct dispatch did not take effect"
    # every packet's hidden arguments sit where the kernel's own code-object metadata says (csrc/codeobj_meta.h), not at assumed offsets
    assert gr.direct_meta_packets() == gr.direct_packets(), (gr.direct_meta_packets(), gr.direct_packets())
    got = _resident(gr, x, 3)
    for w, o in zip(want, got):
        assert np.array_equal(w, o)
    # the stream-ordered entry points still work on the same graph, before and after more direct passes
    gr.set_input(x)
    got2 = gr.run()
    for w, o in zip(want, got2):
        assert np.array_equal(w, o)
    x2 = models.synth_input(g, 78, NP[dtype])
    got3 = _resident(gr, x2, 2)
    gr.close()
    ref = capi.Graph(b)
    want3 = _resident(ref, x2, 1)
    ref.close()
    for w, o in zip(want3, got3):
        assert np.array_equal(w, o)
    assert any(not np.array_equal(a, c) for a, c in zip(want, want3))


def test_direct_dispatch_against_the_oracle_and_the_clock():
    g = models.build("mobilenet_v1", "int8", 1)
    x = models.synth_input(g, 5, DT_INT8)
    want = oracle.run_graph(g, x)
    b = tm2.write_tm2(g)
    gr = capi.Graph(b, direct_dispatch=True)
    got = _resident(gr, x, 2)
    for w, o in zip(want, got):
        assert np.array_equal(o.reshape(w.shape), w)
    gr.time_launches(50)
    t_direct = min(gr.time_launches(300) for _ in range(3)) / 300
    gr.close()
    ref = capi.Graph(b)
    _resident(ref, x, 1)
    ref.time_launches(50)
    t_graph = min(ref.time_launches(300) for _ in range(3)) / 300
    ref.close()
    print("mobilenet_v1 int8 b1: direct %.1f us/step, hipGraph %.1f us/step" % (t_direct * 1e3, t_graph * 1e3))
    assert t_direct < t_graph * 1.02, (t_direct, t_graph)


def test_direct_dispatch_env_switch(monkeypatch):
    g = models.build("mobilenet_v1", "int8", 1)
    b = tm2.write_tm2(g)
    monkeypatch.setenv("TAMD_DIRECT_DISPATCH", "1")
    gr = capi.Graph(b)
    assert gr.direct_packets() > 0
    gr.close()
    monkeypatch.setenv("TAMD_DIRECT_DISPATCH", "0")
    gr = capi.Graph(b, direct_dispatch=True)
    assert gr.direct_packets() == 0
    gr.close()


@pytest.mark.parametrize("batch", [1, 4])
def test_direct_dispatch_coherent_launches_never_serve_stale_tensors(batch):
    """Under direct dispatch the pointwise+depthwise family runs its COHERENT instances (agent-scope loads, write-through
    stores) and their packets carry no fences.  Every pass rewrites the same tensors at the same addresses, so a stale L1 / L2
    line would show as the PREVIOUS input's result: alternate two inputs over many bursts of several passes."""
    g = models.build("mobilenet_v1", "int8", batch)
    b = tm2.write_tm2(g)
    xs = [models.synth_input(g, 300 + i, DT_INT8) for i in range(3)]
    ref = capi.Graph(b)
    wants = [_resident(ref, x, 1) for x in xs]
    ref.close()
    assert not np.array_equal(wants[0][0], wants[1][0])
    gr = capi.Graph(b, direct_dispatch=True)
    assert gr.direct_packets() > 0
    for it in range(90):
        k = (it * 7 + it // 3) % 3
        got = _resident(gr, xs[k], 1 + it % 4)
        assert np.array_equal(got[0], wants[k][0]), "burst %d (input %d)" % (it, k)
    got = _resident(gr, xs[1], 300)          # one long burst
    assert np.array_equal(got[0], wants[1][0])
    gr.close()


def test_direct_dispatch_coherent_kernels_with_fences_kept(monkeypatch):
    monkeypatch.setenv("TAMD_PIN", "direct_coherent=0")      # the same coherent instances behind agent-scope fences
    g = models.build("mobilenet_v1", "int8", 1)
    x = models.synth_input(g, 9, DT_INT8)
    want = oracle.run_graph(g, x)
    gr = capi.Graph(tm2.write_tm2(g), direct_dispatch=True)
    got = _resident(gr, x, 5)
    gr.close()
    for w, o in zip(want, got):
        assert np.array_equal(o.reshape(w.shape), w)


# (packets without the AQL barrier bit -- independent launches inside a pass, the first launch of pass k+1 beside the end of pass k --
#  bought 0.5 - 4 % / nothing on this stack, profiles/r03_*: the dependency analysis stays in graph.hip, the switches that enabled it
#  exist in -DTAMD_EXPERIMENTS builds only since round 5, and so do their tests' subjects)


@pytest.mark.parametrize("name,dtype,batch", [("mobilenet_v1", "int8", 1), ("yolov3_tiny", "uint8", 1)])
def test_device_copy_of_the_outputs_after_a_zero_copy_run(name, dtype, batch):
    """tamd_graph_run on the direct path stores the outputs straight into the pinned host buffers (no download launch): the
    device-side copy -- tamd_graph_output_device (the RCCL gather reads it), tamd_graph_download_outputs -- must still be THIS
    run's bytes, not the previous pass's (it used to be stale)."""
    g = models.build(name, dtype, batch, device_only=(name != "mobilenet_v1"))
    b = tm2.write_tm2(g)
    gr = capi.Graph(b, direct_dispatch=True)
    x1, x2 = models.synth_input(g, 31, NP[dtype]), models.synth_input(g, 32, NP[dtype])
    first = _resident(gr, x1, 1)                  # the staging buffers now hold x1's outputs
    gr.set_input(x2)
    got = [o.copy() for o in gr.run()]            # host-to-host, zero-copy outputs
    assert any(not np.array_equal(a, c) for a, c in zip(first, got))
    again = gr.download()                         # no pass in between: must be x2's outputs
    for a, c in zip(got, again):
        assert np.array_equal(a, c)
    # The raw device pointer is read back through the HIP runtime the LIBRARY is bound to: dlsym on the library's own handle walks its
    # dependency tree (libamdhip64.so.7 of /opt/rocm).  Round 5's one "unexplained" failure of this test was this line, not the product:
    # it said C.CDLL("libamdhip64.so"), and once anything in the process has imported torch AFTER the library was loaded (models.build
    # calibrating an uncached model does: test_gpu_plan_cache.py / test_gpu_baseline_batches.py in front of this file), that NAME
    # resolves to torch's bundled copy under torch/lib -- a second, uninitialised HIP + HSA runtime in the process, whose hipMemcpy
    # answered 100 (hipErrorNoDevice).  Reproduced on the first try with round 5's subset (profiles/r06_zero_copy_flake.txt); the order
    # is forced here (torch imported after the library) so that the wrong handle fails every time, not once per test order.
    capi.lib()
    import torch  # noqa: F401
    hip = hip_runtime_of_the_library()

    def device_copy_is(wants):
        for i, want in enumerate(wants):
            p, n = gr.output_device(i)
            assert n == want.nbytes
            host = np.empty_like(want)
            assert hip.hipMemcpy(host.ctypes.data, p, n, 2) == 0      # hipMemcpyDeviceToHost
            assert np.array_equal(host, want), "output %d: the device copy is not the last run's" % i

    device_copy_is(got)
    # the asynchronous pair: the newest run decides.  It sat in I/O slot 1 (x1's run in I/O slot 0), and both the host copy and the
    # device copy are refreshed from THAT slot's pinned buffers
    gr.set_input(x1)
    gr.run_async()
    gr.set_input(x2)
    gr.run_async()
    gr.wait()
    gr.wait()
    for a, c in zip(got, gr.download()):
        assert np.array_equal(a, c)
    device_copy_is(got)
    # ... and one more asynchronous run is in I/O slot 0 again
    gr.set_input(x1)
    gr.run_async()
    gr.wait()
    device_copy_is(first)
    gr.close()


def test_direct_timestamps_account_for_the_step():
    """round 6: the directly dispatched pass under the HSA runtime's own dispatch profiling (tamd_graph_direct_timestamps) -- one stamp
    pair per packet, no tool in the process.  The packets' durations and the gaps between them add up to (about) the step the host's
    clock sees, every duration is positive, and the passes leave the same bytes behind as any other pass."""
    g = models.build("mobilenet_v1", "int8", 1)
    x = models.synth_input(g, 5, DT_INT8)
    want = oracle.run_graph(g, x)
    gr = capi.Graph(tm2.write_tm2(g), direct_dispatch=True)
    _resident(gr, x, 2)
    gr.time_launches(50)
    step_us = min(1e3 * gr.time_launches(300) / 300 for _ in range(3))
    rows = gr.direct_timestamps(100)
    assert len(rows) == gr.direct_packets() > 0
    assert all(d > 0.2 for _, d, _ in rows), rows
    assert all(gp > -0.05 for _, _, gp in rows), rows                    # in-order, barrier bit on every packet: no overlap
    total = sum(d + gp for _, d, gp in rows)
    print("direct path, HSA stamps: %.2f us per pass (durations %.2f + gaps %.2f); host clock %.2f us" % (total, sum(r[1] for r in rows), sum(r[2] for r in rows), step_us))
    assert 0.7 * step_us < total < 1.5 * step_us, (total, step_us)
    gr.sync()
    got = gr.download()
    gr.close()
    for w, o in zip(want, got):
        assert np.array_equal(o.reshape(w.shape), w)
