"""The drop-in boundary: the unmodified reference library loads our device plugin with
load_tengine_plugin(), `set_context_device(ctx, "HIP", ...)` selects it and create_graph / prerun /
run_graph work unchanged.  CPU part: registration + loud failure without a GPU.  GPU part: the same
tmfile on device "HIP" and on the reference CPU device, byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import conv_graph, eltwise_relu_graph
from tengine_amd import capi, models, tm2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# built where the reference headers exist; the copy under oracle/_ref/ is the one that travels with the prebuilt reference
PLUGIN = next((p for p in (os.path.join(ROOT, d, "libtengine_hip_device.so") for d in (os.path.join("tengine_amd", "lib"), os.path.join("oracle", "_ref")))
               if os.path.exists(p)), os.path.join(ROOT, "tengine_amd", "lib", "libtengine_hip_device.so"))

_loaded = False


def _load_plugin(ref):
    global _loaded
    if not os.path.exists(PLUGIN):
        pytest.skip("plugin not built (needs the reference headers once)")
    L = ref.lib()
    if not _loaded:
        rc = L.load_tengine_plugin(b"hip", PLUGIN.encode(), b"register_hip_device")
        assert rc == 0, "load_tengine_plugin failed"
        _loaded = True
    return L


def placement(rg):
    """[(device name, nodes, nodes that are not Input/Const, [operator names])] per subgraph of a prerun reference graph, asked of
    the plugin (hip_device_placement walks the reference's own graph->subgraph_list)."""
    P = C.CDLL(PLUGIN)
    P.hip_device_placement.restype = C.c_int
    P.hip_device_placement.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    buf = C.create_string_buffer(1 << 16)
    n = P.hip_device_placement(rg.g, buf, len(buf))
    assert n >= 1, n
    out = []
    for line in buf.value.decode().strip().split("\n"):
        f = line.split(" ")
        out.append((f[1], int(f[2]), int(f[3]), f[4].split(",") if len(f) > 4 and f[4] else []))
    assert len(out) == n
    return out


def assert_all_on_hip(rg):
    """every node that is not an Input / Const sits in a subgraph of device "HIP" (no silent CPU fallback)"""
    pl = placement(rg)
    assert sum(real for dev, _, real, _ in pl if dev != "HIP") == 0, pl
    assert sum(real for dev, _, real, _ in pl if dev == "HIP") >= 1, pl
    return pl


class HipOpt(C.Structure):   # == tamd_options; first field dev_name by the reference's convention
    _fields_ = [("dev_name", C.c_char_p), ("size", C.c_int), ("gpu_index", C.c_int), ("use_hip_graph", C.c_int), ("profile", C.c_int)]


def test_plugin_registers_and_is_selectable(ref):
    L = _load_plugin(ref)
    ctx = L.create_context(b"t", 1)
    opt = HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0)
    assert L.set_context_device(ctx, b"HIP", C.byref(opt), C.sizeof(opt)) == 0
    assert L.set_context_device(ctx, b"NOPE", None, 0) != 0


def test_plugin_without_gpu_fails_loudly_not_silently(ref):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    _load_plugin(ref)
    g, x = conv_graph(3, 1, 16, 8, 8, 16, 1)
    rg = ref.RefGraph(tm2.write_tm2(g), ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    with pytest.raises(RuntimeError):
        rg.prerun()


def _split_only(ref, g, x, mode):
    """placement after the splitter ran; without a GPU the device pre_run that follows it fails (loudly), the split stays readable"""
    rg = ref.RefGraph(tm2.write_tm2(g), mode, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    try:
        rg.prerun()
    except RuntimeError:
        assert capi.device_count() == 0
    pl = placement(rg)
    rg.close()
    return pl


def _add_cpu_only_tail(g):
    """appends a node the device refuses (tamd_node_supported: int8 Softmax runs over axes >= 1) and the reference's CPU device runs:
    a Softmax over the BATCH axis (softmax_kernel_ref_int8.c is axis-agnostic) -- with two images its bytes depend on the data, so a
    wrong hand-over shows"""
    y = g.nodes[-1].outputs[0]
    o = g.add_tensor("prob", list(g.tensors[y].dims), tm2.DT_INT8, tm2.TT_VAR, None, [1.0 / 127.0], [0])
    g.output_nodes = [g.add_node("softmax", "Softmax", [y], [o], axis=0)]


def test_split_keeps_whole_ssd_on_the_device(ref):
    """Concat(axis 2) of the priors used to send ALL of MobileNet-SSD to the CPU device, and no test saw it"""
    _load_plugin(ref)
    g = models.build("mssd", "uint8", 1, tail=True, priorbox=True)
    pl = _split_only(ref, g, models.synth_input(g, 5, tm2.DT_UINT8), ref.MODE_UINT8)
    assert len(pl) == 1 and pl[0][0] == "HIP", pl
    ops = pl[0][3]
    assert ops.count("PriorBox") == 6 and ops.count("Concat") == 3 and "Softmax" in ops and ops.count("Convolution") == 47, pl


def test_split_keeps_whole_int8_ssd_on_the_device(ref):
    """round 6 (VERDICT r5 missing #4): the int8 forms of Permute / Flatten / Reshape / PriorBox / Softmax(axis 2) / Concat(axis 2) run
    on the device, so an int8 MobileNet-SSD no longer ping-pongs to the CPU device: ONE "HIP" subgraph up to detection_output's inputs"""
    _load_plugin(ref)
    g = models.build("mssd", "int8", 1, tail=True, priorbox=True)
    pl = _split_only(ref, g, models.synth_input(g, 5, tm2.DT_INT8), ref.MODE_INT8)
    assert len(pl) == 1 and pl[0][0] == "HIP", pl
    ops = pl[0][3]
    assert ops.count("PriorBox") == 6 and ops.count("Concat") == 3 and ops.count("Permute") == 12 and "Softmax" in ops and "Reshape" in ops, pl
    assert ops.count("Convolution") == 47, pl


def test_split_leaves_a_consumer_of_a_dense_int8_tensor_to_the_cpu(ref):
    """round 6: conv -> Permute -> Flatten -> FullyConnected (int8).  Permute / Flatten run on the device and leave a DENSE tensor there; an
    FC is not one of the operators that may re-read it (csrc/graph_plan.hip), so the splitter keeps it on the CPU device instead of
    handing the planner a graph it refuses"""
    from helpers import I8_HEAD_CASES, i8_head_graph
    _load_plugin(ref)
    g, x = i8_head_graph(**dict(I8_HEAD_CASES["standalone_permute"], n=1))
    pm = g.nodes[g.output_nodes[0]].outputs[0]
    d = g.tensors[pm].dims
    hidden = d[1] * d[2] * d[3]
    fl = g.add_tensor("flat", [d[0], hidden], tm2.DT_INT8, tm2.TT_VAR, None, list(g.tensors[pm].scales), [0])
    g.add_node("flat", "Flatten", [pm], [fl], axis=1, end_axis=3)
    rng = np.random.default_rng(2)
    w = g.add_const("fc_w", rng.integers(-127, 128, size=(10, hidden)).astype(np.int8), tm2.DT_INT8, [0.01] * 10, [0] * 10)
    y = g.add_tensor("fc", [d[0], 10], tm2.DT_INT8, tm2.TT_VAR, None, [0.5], [0])
    g.output_nodes = [g.add_node("fc", "FullyConnected", [fl, w], [y], num_output=10)]
    pl = _split_only(ref, g, x, ref.MODE_INT8)
    hip_ops = [o for dev, _, _, ops in pl if dev == "HIP" for o in ops if o not in ("InputOp", "Const")]
    cpu_ops = [o for dev, _, _, ops in pl if dev != "HIP" for o in ops if o not in ("InputOp", "Const")]
    assert "FullyConnected" in cpu_ops and "Convolution" in hip_ops and "Permute" in hip_ops, pl


def test_split_keeps_whole_resnet50_int8_on_the_device(ref):
    """round 4: the benchmark graph of BASELINE configs[2] ends in an int8 Softmax; with softmax_i8 on the
    device it is ONE "HIP" subgraph -- no CPU tail, so run_graph(g, 0) pipelines it like MobileNet"""
    _load_plugin(ref)
    g = models.build("resnet50", "int8", 1)
    assert g.nodes[-1].op == "Softmax"
    pl = _split_only(ref, g, models.synth_input(g, 5), ref.MODE_INT8)
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert len(real) == 1 and real[0][0] == "HIP", pl
    assert real[0][1].count("Convolution") == 53 and real[0][1][-1] == "Softmax", pl


BASELINE_GRAPHS = [("squeezenet_v1.1", "fp32", {}), ("mobilenet_v1", "int8", {}), ("resnet50", "int8", {}), ("yolov3_tiny", "uint8", {}),
                   ("mssd", "uint8", {})]


@pytest.mark.parametrize("name,dtype,kw", BASELINE_GRAPHS, ids=[b[0] for b in BASELINE_GRAPHS])
def test_split_gives_every_baseline_graph_to_the_device_whole(ref, name, dtype, kw):
    """the five BASELINE config graphs as tengine_amd.models builds them (SURVEY appendix C census): after hip_split_graph every
    compute node sits in ONE subgraph of device "HIP" -- no CPU piece, hence no hand-over inside a run (checked without a GPU: the
    split happens before the device is touched)"""
    _load_plugin(ref)
    g = models.build(name, dtype, 1, **kw)
    dt = {"fp32": tm2.DT_FP32, "int8": tm2.DT_INT8, "uint8": tm2.DT_UINT8}[dtype]
    mode = {"fp32": ref.MODE_FP32, "int8": ref.MODE_INT8, "uint8": ref.MODE_UINT8}[dtype]
    pl = _split_only(ref, g, models.synth_input(g, 5, dt), mode)
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert len(real) == 1 and real[0][0] == "HIP", pl
    want = sorted(n.op for n in g.nodes if n.op not in ("InputOp", "Const"))
    assert sorted(o for o in real[0][1] if o not in ("InputOp", "Const")) == want, (real[0][1], want)


def test_split_cuts_around_an_unsupported_node_instead_of_surrendering(ref):
    """conv -> int8 Softmax over the BATCH axis (not on the device: tamd_node_supported takes axes >= 1 -- until round 5 this test used
    the rows of the map, which the device runs since round 6) -> conv: the two convolutions stay on "HIP", only the softmax goes to the CPU"""
    _load_plugin(ref)
    g, x = conv_graph(5, 1, 32, 6, 6, 16, 1, act=-1)
    y = g.nodes[-1].outputs[0]
    o = g.add_tensor("prob", list(g.tensors[y].dims), tm2.DT_INT8, tm2.TT_VAR, None, [1.0 / 127.0], [0])
    g.add_node("softmax", "Softmax", [y], [o], axis=0)
    rng = np.random.default_rng(1)
    w2 = g.add_const("w2", rng.integers(-127, 128, size=(8, 16, 1, 1)).astype(np.int8), tm2.DT_INT8, [0.01] * 8, [0] * 8)
    o2 = g.add_tensor("out2", [1, 8, 6, 6], tm2.DT_INT8, tm2.TT_VAR, None, [0.02], [0])
    ni = g.add_node("conv2", "Convolution", [o, w2], [o2], kernel_h=1, kernel_w=1, stride_h=1, stride_w=1, dilation_h=1, dilation_w=1,
                    input_channel=16, output_channel=8, group=1, activation=-1, pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
    g.output_nodes = [ni]
    pl = _split_only(ref, g, x, ref.MODE_INT8)
    assert [(dev, ops) for dev, _, _, ops in pl if ops] == [("HIP", ["Convolution"]), (pl[1][0], ["Softmax"]), ("HIP", ["Convolution"])], pl
    assert pl[1][0] != "HIP"


def test_split_leaves_an_int8_relu6_to_the_cpu(ref):
    """conv -> ReLU6 in int8: ReLU6 is in the plugin's operator table, the library has it for fp32 alone (tamd_op_supported) -- the
    convolution stays on "HIP", the ReLU6 goes to the CPU device"""
    _load_plugin(ref)
    g, x = conv_graph(6, 1, 16, 6, 6, 16, 1, act=-1)
    y = g.nodes[-1].outputs[0]
    o = g.add_tensor("r6", list(g.tensors[y].dims), tm2.DT_INT8, tm2.TT_VAR, None, list(g.tensors[y].scales), [0])
    g.output_nodes = [g.add_node("relu6", "ReLU6", [y], [o])]
    pl = _split_only(ref, g, x, ref.MODE_INT8)
    assert [(dev, ops) for dev, _, _, ops in pl if ops] == [("HIP", ["Convolution"]), (pl[1][0], ["ReLU6"])], pl
    assert pl[1][0] != "HIP"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["conv3x3", "resblock_tail", "resnet50_prob", "mobilenet_v1"])
def test_hip_device_equals_reference_cpu_device(ref, case):
    _load_plugin(ref)
    if case == "conv3x3":
        g, x = conv_graph(31, 2, 64, 20, 20, 96, 3, 1, 1)
    elif case == "resblock_tail":
        g, x = eltwise_relu_graph(9, 2, 64, 14, 14, True)
    elif case == "resnet50_prob":          # the whole benchmark graph, its int8 Softmax included, all on "HIP"
        g = models.build("resnet50", "int8", 1)
        x = models.synth_input(g, 8)
    else:
        g = models.build("mobilenet_v1", "int8", 1)
        x = models.synth_input(g, 7)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 4)
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    assert_all_on_hip(rg)
    got = rg.outputs()
    rg.run()                       # second run re-reads the input pointer, replays the hipGraph
    again = rg.outputs()
    rg.close()
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)


def _split_count():
    P = C.CDLL(PLUGIN)
    P.hip_device_split_subgraphs.restype = C.c_int
    return P.hip_device_split_subgraphs()


@pytest.mark.gpu
@pytest.mark.parametrize("case,env,split", [("conv3x3_b2", "2", True), ("mobilenet_v1_b2", "2", True), ("resblock_tail_b2", "2", True), ("resnet50_prob_b2", "2", True),
                                            ("mobilenet_v1_b16", None, True), ("mobilenet_v1_b16", "0", False), ("conv3x3_b2", None, False),
                                            ("conv3x3_b8", None, True), ("conv3x3_b6", None, False),
                                            ("conv3x3_b3", "2", False)])
def test_batched_subgraph_as_two_half_batch_graphs(ref, case, env, split, monkeypatch):
    """round 6: a subgraph of batch-wise independent operators whose activations all carry an even batch runs as TWO device graphs of half
    the batch, side by side on their own queues (from batch 8 on; TAMD_SPLIT_BATCH=2: wherever possible, =0: never): the reference CPU
    device's bytes either way, on the first run and on a second one (input pointers re-read), and the split is asserted, not assumed."""
    _load_plugin(ref)
    if env is None:
        monkeypatch.delenv("TAMD_SPLIT_BATCH", raising=False)
    else:
        monkeypatch.setenv("TAMD_SPLIT_BATCH", env)
    if case.startswith("conv3x3"):
        g, x = conv_graph(31, int(case[-1]), 64, 20, 20, 96, 3, 1, 1)      # (batch = the case's last digit: 2, 3, 6, 8)
    elif case == "resblock_tail_b2":
        g, x = eltwise_relu_graph(9, 2, 64, 14, 14, True)
    elif case == "resnet50_prob_b2":
        g = models.build("resnet50", "int8", 2)
        x = models.synth_input(g, 8)
    elif case == "mobilenet_v1_b2":        # halves of ONE image: the depthwise layers must still follow the batch-2 formula of the reference
        g = models.build("mobilenet_v1", "int8", 2)
        x = models.synth_input(g, 7)
    else:
        g = models.build("mobilenet_v1", "int8", 16)
        x = models.synth_input(g, 7)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 4)
    before = _split_count()
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    assert_all_on_hip(rg)
    assert (_split_count() - before >= 1) == split, (case, env, _split_count() - before)
    got = rg.outputs()
    rg.run()
    again = rg.outputs()
    rg.close()
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)


@pytest.mark.gpu
def test_unsupported_tail_falls_back_to_cpu_subgraph(ref):
    """int8 graph with a tail the device does not run -- a Softmax over the batch axis; until round 5 this test used the rows of the map,
    which the device runs since round 6: the splitter gives conv->HIP, softmax->CPU (SURVEY §7 'subgraph ping-pong')."""
    _load_plugin(ref)
    g, x = conv_graph(5, 2, 32, 6, 6, 10, 1, act=-1)
    _add_cpu_only_tail(g)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 1)[0]
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = placement(rg)
    got = rg.outputs()[0]
    rg.close()
    assert np.array_equal(want, got)
    # conv on "HIP", the int8 softmax on the CPU device -- and nothing else anywhere
    hip_ops = [o for dev, _, _, ops in pl if dev == "HIP" for o in ops]
    cpu_ops = [o for dev, _, _, ops in pl if dev != "HIP" for o in ops]
    assert hip_ops == ["Convolution"] and cpu_ops == ["Softmax"], pl


@pytest.mark.gpu
def test_hip_device_fp32_matches_reference_cpu_device(ref):
    """fp32: SqueezeNet-v1.1 through the reference's API on device "HIP" vs its CPU device
    (im2col+sgemm / Winograd there, fp32 MFMA here): 1e-4."""
    _load_plugin(ref)
    g = models.build("squeezenet_v1.1", "fp32", 1)
    x = models.synth_input(g, 5, tm2.DT_FP32)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_FP32, 8)[0]
    rg = ref.RefGraph(b, ref.MODE_FP32, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    assert_all_on_hip(rg)
    got = rg.outputs()[0]
    rg.close()
    assert np.abs(got - want).max() <= 1e-4, np.abs(got - want).max()       # absolute, as north_star states it
    assert abs(float(got.sum()) - 1.0) < 1e-3          # softmax ran (on the device)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["route", "yolov3_tiny", "ssd_head", "mssd", "mssd_tail", "mssd_full", "priorbox"])
def test_hip_device_uint8_equals_reference_cpu_device(ref, case):
    """uint8 through the reference's own API: device "HIP" == CPU device, byte for byte."""
    from helpers import u8_route_graph
    _load_plugin(ref)
    if case == "route":
        g, x = u8_route_graph(16, 2, 8, 6, 6)
    elif case == "ssd_head":
        from helpers import u8_ssd_head_graph
        g, x = u8_ssd_head_graph(17, 2, 16, 6, 6)
    elif case in ("mssd", "mssd_tail"):      # _tail: + Reshape -> Softmax -> Flatten on mbox_conf, all on "HIP"
        g = models.build("mssd", "uint8", 1, tail=(case == "mssd_tail"))
        x = models.synth_input(g, 5, tm2.DT_UINT8)
    elif case == "mssd_full":                # + the six PriorBox nodes and their Concat: the graph ends at detection_output's inputs
        g = models.build("mssd", "uint8", 1, tail=True, priorbox=True)
        x = models.synth_input(g, 5, tm2.DT_UINT8)
    elif case == "priorbox":                 # non-square image, fractional sizes, clip; the concat of the priors re-quantises
        from helpers import PRIORBOX_CASES, priorbox_graph
        g, x = priorbox_graph(dtype=tm2.DT_UINT8, **PRIORBOX_CASES["non_square_fractional_sizes_clip"])
    else:
        g = models.build("yolov3_tiny", "uint8", 1)
        x = models.synth_input(g, 3, tm2.DT_UINT8)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_UINT8, 8)
    rg = ref.RefGraph(b, ref.MODE_UINT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = assert_all_on_hip(rg)          # incl. mssd_full / priorbox: Concat(axis 2) of the priors stays on the device
    assert len(pl) == 1, pl
    got = rg.outputs()
    rg.close()
    assert len(want) == len(got)
    for w, o in zip(want, got):
        assert np.array_equal(w, o)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ssd_head", "mssd_full", "priorbox", "softmax_over_h"])
def test_hip_device_int8_head_plumbing_equals_reference_cpu_device(ref, case):
    """round 6: the int8 forms of Permute / Flatten / Reshape / PriorBox / Concat(any axis) / Softmax(any axis >= 1) through the reference's
    own API: ONE "HIP" subgraph, the CPU device's bytes"""
    from helpers import I8_HEAD_CASES, PRIORBOX_CASES, i8_head_graph, priorbox_graph
    _load_plugin(ref)
    if case == "mssd_full":
        g = models.build("mssd", "int8", 1, tail=True, priorbox=True)
        x = models.synth_input(g, 5, tm2.DT_INT8)
    elif case == "priorbox":
        g, x = priorbox_graph(dtype=tm2.DT_INT8, **PRIORBOX_CASES["non_square_fractional_sizes_clip"])
    elif case == "ssd_head":
        g, x = i8_head_graph(**I8_HEAD_CASES["ssd_head_two_maps"])
    else:
        g, x = i8_head_graph(**I8_HEAD_CASES[case])
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 8)
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = assert_all_on_hip(rg)
    assert len(pl) == 1, pl
    got = rg.outputs()
    rg.close()
    assert len(want) == len(got)
    for w, o in zip(want, got):
        assert np.array_equal(w, o)


@pytest.mark.gpu
def test_int8_rescaling_concat_runs_on_the_device_and_matches_cpu(ref):
    """an int8 concat whose inputs carry their own scales / ragged channel counts used to fail
    prerun_graph on "HIP"; now the device copies with the reference's re-scaling arithmetic"""
    import importlib
    glue = importlib.import_module("test_gpu_glue_int8")
    _load_plugin(ref)
    g, x = glue._two_branch_concat(52, 1, 16, 6, 7, 20, 12)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 2)[0]
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    assert_all_on_hip(rg)
    got = rg.outputs()[0]
    rg.close()
    assert np.array_equal(want, got)


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["conv", "mobilenet_v1", "conv_split"])
def test_async_run_graph_through_the_plugins_scheduler(ref, model, monkeypatch):
    """SURVEY 8(f)4, the scheduler half: the reference's own run_graph(graph, 0) reaches interface.async_run through the scheduler
    the plugin installs on the context; two runs in flight, a third is refused; results in submission order, reference bytes.
    wait_graph() itself cannot work in the unmodified reference (its status test is always true, c_api.c:588): asserted as is,
    and hip_wait_graph() -- the body it was meant to have -- collects the runs."""
    L = _load_plugin(ref)
    P = C.CDLL(PLUGIN)
    P.hip_wait_graph.restype = C.c_int
    P.hip_wait_graph.argtypes = [C.c_void_p, C.c_int]
    L.wait_graph.restype = C.c_int
    L.wait_graph.argtypes = [C.c_void_p, C.c_int]
    if model == "conv_split":                      # (round 6) the same protocol on a subgraph that runs as two half-batch graphs
        monkeypatch.setenv("TAMD_SPLIT_BATCH", "2")
    if model in ("conv", "conv_split"):
        g, x1 = conv_graph(61, 2, 64, 14, 14, 96, 3, 1, 1)
    else:
        g = models.build("mobilenet_v1", "int8", 1)
        x1 = models.synth_input(g, 7)
    rng = np.random.default_rng(5)
    x2 = rng.integers(-127, 128, size=x1.shape).astype(np.int8)
    b = tm2.write_tm2(g)
    want1 = ref.run_model(b, x1, ref.MODE_INT8, 4)[0]
    want2 = ref.run_model(b, x2, ref.MODE_INT8, 4)[0]
    assert not np.array_equal(want1, want2)
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    before = _split_count()
    rg.set_input(x1)
    rg.prerun()
    assert_all_on_hip(rg)
    assert (_split_count() - before >= 1) == (model == "conv_split")
    buf = np.ascontiguousarray(x1).copy()           # ONE application buffer, refilled between submissions
    t = L.get_graph_input_tensor(rg.g, 0, 0)
    assert L.set_tensor_buffer(t, buf.ctypes.data, buf.nbytes) == 0
    for rep in range(3):
        buf[...] = x1
        assert L.run_graph(rg.g, 0) == 0            # non-blocking: returns with the run in flight
        buf[...] = x2                               # the input was staged at submission: the buffer is the application's again
        assert L.run_graph(rg.g, 0) == 0
        assert L.run_graph(rg.g, 0) != 0            # a third run in flight is refused
        assert L.wait_graph(rg.g, 1) == -1          # the reference's own wait_graph: always -1 (c_api.c:588)
        assert P.hip_wait_graph(rg.g, 1) == 0
        assert np.array_equal(rg.outputs()[0], want1)
        assert P.hip_wait_graph(rg.g, 1) == 0
        assert np.array_equal(rg.outputs()[0], want2)
    buf[...] = x1
    assert L.run_graph(rg.g, 1) == 0                # and the blocking run still works on the same graph
    assert np.array_equal(rg.outputs()[0], want1)
    rg.close()


@pytest.mark.gpu
def test_async_runs_of_a_mixed_graph_pipeline_its_hip_piece_and_finish_the_cpu_tail_at_wait(ref):
    """a graph that is one leading "HIP" subgraph + CPU pieces behind it (an SSD model's DetectionOutput; here an
    int8 Softmax over the batch axis) used to run blocking under run_graph(g, 0).  Now the HIP piece is submitted asynchronously (two in flight) and
    hip_wait_graph delivers the oldest run's device outputs, then runs the CPU tail on them -- reference bytes, submission order."""
    L = _load_plugin(ref)
    P = C.CDLL(PLUGIN)
    P.hip_wait_graph.restype = C.c_int
    P.hip_wait_graph.argtypes = [C.c_void_p, C.c_int]
    g, x1 = conv_graph(5, 2, 32, 6, 6, 10, 1, act=-1)
    _add_cpu_only_tail(g)                                             # a CPU-device node behind the convolution
    b = tm2.write_tm2(g)
    x2 = np.random.default_rng(3).integers(-127, 128, size=x1.shape).astype(np.int8)
    want1 = ref.run_model(b, x1, ref.MODE_INT8, 1)[0]
    want2 = ref.run_model(b, x2, ref.MODE_INT8, 1)[0]
    assert not np.array_equal(want1, want2)
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
    rg.set_input(x1)
    rg.prerun()
    pl = placement(rg)
    assert [dev for dev, _, real, _ in pl if real].count("HIP") == 1 and len([1 for dev, _, real, _ in pl if real]) == 2, pl
    buf = np.ascontiguousarray(x1).copy()
    t = L.get_graph_input_tensor(rg.g, 0, 0)
    assert L.set_tensor_buffer(t, buf.ctypes.data, buf.nbytes) == 0
    for rep in range(3):
        buf[...] = x1
        assert L.run_graph(rg.g, 0) == 0
        buf[...] = x2
        assert L.run_graph(rg.g, 0) == 0
        assert L.run_graph(rg.g, 0) != 0            # two in flight: the third is refused, so the runs really are asynchronous
        assert P.hip_wait_graph(rg.g, 1) == 0
        assert np.array_equal(rg.outputs()[0], want1)
        assert P.hip_wait_graph(rg.g, 1) == 0
        assert np.array_equal(rg.outputs()[0], want2)
    buf[...] = x1
    assert L.run_graph(rg.g, 1) == 0
    assert np.array_equal(rg.outputs()[0], want1)
    rg.close()


@pytest.mark.gpu
def test_the_contexts_scheduler_is_the_references_again_after_the_last_hip_graph(ref):
    """hip_split_graph installs the plugin's scheduler on the context; when the last graph that was pre-run through it
    is post-run the reference's own scheduler is back (a context must not keep pointing into a library that may be unloaded),
    and a graph pre-run later on a fresh HIP context pipelines again."""
    L = _load_plugin(ref)
    P = C.CDLL(PLUGIN)
    P.hip_wait_graph.restype = C.c_int
    P.hip_wait_graph.argtypes = [C.c_void_p, C.c_int]
    g, x = conv_graph(8, 1, 32, 8, 8, 32, 1)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 1)[0]
    for _ in range(2):
        rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=HipOpt(b"HIP", C.sizeof(HipOpt), 0, 1, 0))
        rg.set_input(x)
        rg.prerun()
        assert L.run_graph(rg.g, 0) == 0            # the plugin's scheduler is on this context
        assert P.hip_wait_graph(rg.g, 1) == 0
        assert np.array_equal(rg.outputs()[0], want)
        rg.close()                                  # postrun: the last live graph of the context -> default scheduler restored


class ShortOpt(C.Structure):     # an application that only knows the reference's convention: first field dev_name
    _fields_ = [("dev_name", C.c_char_p), ("size", C.c_int)]


@pytest.mark.gpu
def test_short_option_blob_is_not_over_read(ref):
    _load_plugin(ref)
    g, x = conv_graph(33, 1, 32, 10, 10, 48, 3, 1, 1)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 1)[0]
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=ShortOpt(b"HIP", C.sizeof(ShortOpt)))
    rg.set_input(x)
    rg.run()
    assert_all_on_hip(rg)
    got = rg.outputs()[0]
    rg.close()
    assert np.array_equal(want, got)
