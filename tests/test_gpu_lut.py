"""Quantised Sigmoid / Clip / HardSwish / Mish on the device (csrc/lut_tables.cc + misc_kernels.hip: lut_u8): device bytes == the real
reference library's bytes on the same tmfile, through the C ABI with pooled tensors (the default) and with keep_tensors = 1, and
through the plugin.  The shapes are the smallest at which the kernel can go wrong: int8 tensors with padding lanes in front of a
convolution that reads them, byte counts that are no multiple of the 16 a thread moves, several blocks with a ragged last one."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import lut_helpers as lh
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(b, x, **kw):
    gr = capi.Graph(b, **kw)
    gr.set_input(x)
    out = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    again = gr.run()                                     # (after the profiling passes: the launches are idempotent)
    gr.close()
    for a, c in zip(out, again):
        assert np.array_equal(a, c)
    return out, names


def _equals_reference(ref, g, x, dtype, lut_launches):
    """pooled and keep_tensors = 1 against the reference on the same bytes; the launch list names lut_u8 once per node"""
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, lh.ref_mode(ref, dtype))
    for keep in (False, True):
        got, names = _device(b, x, keep_tensors=keep)
        assert names.count("lut_u8") == lut_launches, names
        assert len(got) == len(want)
        for w, o in zip(want, got):
            assert w.shape == o.shape and w.dtype == o.dtype
            assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
    return want


@pytest.mark.parametrize("op", ["Sigmoid", "Clip"])
def test_int8_padding_lanes_stay_zero_in_front_of_a_convolution(ref, op):
    """conv1x1 (8 -> 5) -> op -> conv3x3 pad 1 (5 -> 7) at (2, 8, 5, 3): a non-zero padding lane in the op's output changes the second
    convolution's sums (its weights' padding is zero, its input's must be: table[0] is not 0 for Sigmoid)"""
    g, x = lh.padding_graph(op)
    _equals_reference(ref, g, x, DT_INT8, 1)


@pytest.mark.parametrize("op", ["Sigmoid", "Clip"])
@pytest.mark.parametrize("dims", [(1, 16, 1, 1), (1, 5, 3, 3), (2, 17, 5, 3), (1, 24, 33, 31)], ids=lambda d: "x".join(map(str, d)))
def test_int8_shapes_fed_by_the_graph_input(ref, op, dims):
    """one vector; padding lanes; two vectors per pixel, the second nearly all padding; 1023 pixels x 32 bytes = 8 blocks, the last ragged"""
    g = lh.unary_graph(op, DT_INT8, dims, (0.05, 0), (1 / 127.0 if op == "Sigmoid" else 6 / 127.0, 0))
    _equals_reference(ref, g, lh.random_bytes(3, DT_INT8, dims), DT_INT8, 1)


def test_int8_behind_a_fully_connected(ref):
    """FC(2 x 40 -> 10) -> Sigmoid: a 2-D tensor"""
    g, x = lh.fc_sigmoid_graph()
    _equals_reference(ref, g, x, DT_INT8, 1)


@pytest.mark.parametrize("op", ["Sigmoid", "Clip"])
def test_int8_dense_tensor_behind_a_reshape(ref, op):
    """conv -> Reshape -> op: 105 bytes per image in the reference's dense order, no padding, a tail behind the last whole vector"""
    g, x = lh.dense_graph(op)
    _equals_reference(ref, g, x, DT_INT8, 1)


@pytest.mark.parametrize("op", ["Sigmoid", "Clip", "HardSwish", "Mish"])
@pytest.mark.parametrize("dims", [(1, 1, 1, 1), (1, 3, 5, 7), (2, 8, 9, 9), (1, 24, 33, 31)], ids=lambda d: "x".join(map(str, d)))
def test_uint8_shapes(ref, op, dims):
    """one byte; 105 bytes (six vectors and a tail); 1296; 24552 = 5 blocks and 6 bytes"""
    out_q = {"Sigmoid": (1 / 255.0, 0), "Clip": (6 / 255.0, 0), "HardSwish": (0.031, 12), "Mish": (0.031, 12)}[op]
    g = lh.unary_graph(op, DT_UINT8, dims, (0.05, 77), out_q)
    _equals_reference(ref, g, lh.random_bytes(4, DT_UINT8, dims), DT_UINT8, 1)


@pytest.mark.parametrize("build,dtype,luts", [(lh.silu_graph, DT_INT8, 1), (lh.relu6_block_graph, DT_INT8, 2), (lh.mish_pool_graph, DT_UINT8, 1)],
                         ids=["int8-silu", "int8-relu6-block", "uint8-mish-pool"])
def test_patterns(ref, build, dtype, luts):
    g, x = build()
    _equals_reference(ref, g, x, dtype, luts)


def test_mobilenet_v1_int8_batch1_launch_list_is_the_parents(monkeypatch):
    """the new planner code is not on the flagship's path: its launch list is, name for name, the one recorded before this operator
    family existed (tests/golden/mobilenet_v1_int8_b1_kernels.json; TAMD_AUTOTUNE=0 there and here: every site keeps its incumbent, so
    the list does not depend on a plan-time race)"""
    monkeypatch.setenv("TAMD_AUTOTUNE", "0")
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "mobilenet_v1_int8_b1_kernels.json")))
    gr = capi.Graph(tm2.write_tm2(models.build("mobilenet_v1", "int8", 1)), direct_dispatch=True)
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    assert names == want["kernels"] and "lut_u8" not in names


def test_split_batch_on_the_silu_pattern(ref):
    """batch 2 as two device graphs of one image each: the four operators treat the images of a batch independently"""
    g, x = lh.silu_graph((2, 8, 5, 3))
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8)
    outs = []
    for split in (1, 2):
        gr = capi.Graph(b, split_batch=split)
        assert gr.halves() == (2 if split == 2 else 0)
        gr.set_input(x)
        outs.append(gr.run())
        gr.close()
    for w, one, two in zip(want, outs[0], outs[1]):
        assert np.array_equal(one, two) and np.array_equal(w, two)


@pytest.mark.parametrize("build,dtype", [(lh.placement_a, DT_INT8), (lh.placement_b, DT_UINT8)], ids=["int8-clip-sigmoid", "uint8-mish-hardswish"])
def test_plugin_runs_the_graph_as_one_hip_subgraph(ref, build, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  WHERE the operators land is the splitter's decision and is pinned where the plugin is always built from this tree's
    source, next to the reference headers (tests/test_lut_cpu.py).  It is asserted here too -- one "HIP" subgraph -- when the plugin in
    use is the one this tree's build() compiled (tengine_amd/lib/).  The copy under oracle/_ref/ travels with a prebuilt reference to
    machines without those headers and may have been compiled from an older hip_device.cc, whose operator table cannot know the four
    operators: with such a binary each of them is a CPU node between device subgraphs (Convolution | Clip | Convolution | Sigmoid seen),
    the bytes must still be the reference's, and nothing in this tree can change where that binary puts them."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = build(dtype)
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, dtype)
    want = ref.run_model(b, x, mode)
    rg = ref.RefGraph(b, mode, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = tp.placement(rg)
    got = rg.outputs()
    rg.run()
    again = rg.outputs()
    rg.close()
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert real and real[0][0] == "HIP", pl                     # the convolutions are on the device with any plugin
    if built_here:
        assert len(real) == 1, (tp.PLUGIN, pl)
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
