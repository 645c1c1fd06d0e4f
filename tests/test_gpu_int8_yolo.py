"""int8 YOLOv3-tiny whole on the device: the int8 nearest Upsample (upsample_i8: upsample_ref.c's uint8 routine on the int8 bytes),
ReLU -> max-pool as one launch (relu_pool_i8) and the whole graph -- every byte against the REAL reference's CPU device (`ref`),
the 416 x 416 graph against the committed golden of the same reference."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import pinned
from tengine_amd import capi, models, tm2
from yolo_i8_helpers import (RELU_POOL_SCALES, RELU_POOL_SHAPES, all_bytes_inputs, relu_pool_concat_graph, relu_pool_graph,
                             upsample_concat_graph, upsample_graph)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device(g, x, **kw):
    gr = capi.Graph(tm2.write_tm2(g), **kw)
    gr.set_input(x)
    out = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    return out, names


def same(want, got):
    assert len(want) == len(got) >= 1
    for w, o in zip(want, got):
        o = np.asarray(o).reshape(w.shape)
        assert o.dtype == w.dtype and np.array_equal(o, w), "%d of %d bytes differ" % (np.count_nonzero(o != w), w.size)


# ---- Upsample alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", [(0.02, 0.02), (0.013, 0.017), (0.05, 0.02)], ids=["copy", "rescale_up", "rescale_down_saturates"])
@pytest.mark.parametrize("dims,factor", [([2, 5, 3, 4], 2), ([1, 16, 1, 1], 3), ([1, 33, 7, 5], 2)], ids=["tail_batch2", "one_pixel_x3", "two_vectors_plus_one"])
def test_upsample_equals_the_reference_on_every_byte_value(ref, dims, factor, scales):
    g = upsample_graph(dims, factor, *scales)
    b = tm2.write_tm2(g)
    gr = capi.Graph(b)
    assert [k["kernel"] for k in gr.profile(1)] == ["upsample_i8"]
    seen = set()
    for x in all_bytes_inputs(7, dims):
        want = ref.run_model(b, x, ref.MODE_INT8, 1)
        gr.set_input(x)
        same(want, gr.run())
        seen |= set(np.unique(x).tolist())
        if scales[0] != scales[1] and (x < 0).any():
            # the reference reads the BYTES: a negative input is a large unsigned value there, not what a signed rescale would give
            signed = np.clip(np.round(x.astype(np.float32) * np.float32(scales[0]) / np.float32(scales[1])), -127, 127).astype(np.int8)
            assert not np.array_equal(np.repeat(np.repeat(signed, factor, 2), factor, 3), want[0])
    gr.close()
    assert len(seen) == 256


# ---- Upsample into a channel concat --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,kw,copies", [
    ("first_in_place", dict(upsample_first=True), 0),                    # offset 0: upsample_i8 stores into the concat's buffer
    ("second_offset_48_in_place", dict(upsample_first=False), 0),        # offset 48 (a multiple of 16): in place too
    ("second_offset_40_copied", dict(upsample_first=False, side=40), 2),  # offset 40: not 16-byte aligned -> concat_copy_i8 (and 40 channels: the side too)
    ("own_scale_rescaling_copy", dict(upsample_first=True, same_scale=False), 1),
])
def test_upsample_into_a_concat(ref, case, kw, copies):
    g, x = upsample_concat_graph(11, **kw)
    want = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8, 1)
    got, names = device(g, x)
    same(want, got)
    assert names.count("upsample_i8") == 1 and names.count("concat_copy_i8") == copies, names
    assert len(np.unique(want[0])) > 16


# ---- ReLU -> max-pool ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc", sorted(RELU_POOL_SCALES))
@pytest.mark.parametrize("shape", sorted(RELU_POOL_SHAPES))
def test_relu_pool_is_one_launch_and_equals_the_reference(ref, shape, sc):
    dims, k, s, p, caffe = RELU_POOL_SHAPES[shape]
    g, x = relu_pool_graph(21, dims, k, s, p, caffe, *RELU_POOL_SCALES[sc])
    want = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8, 1)
    got, names = device(g, x)
    assert names == ["relu_pool_i8"], names
    same(want, got)
    with pinned(relu_pool=0):
        unfused, names_u = device(g, x)
    assert names_u == ["relu_i8", "pool_i8"], names_u
    same(want, unfused)
    assert len(np.unique(want[0])) > 8


def test_relu_output_of_a_fused_pair_is_refused_by_read_tensor():
    dims, k, s, p, caffe = RELU_POOL_SHAPES["k2s2"]
    g, x = relu_pool_graph(22, dims, k, s, p, caffe, *RELU_POOL_SCALES["leaky0.1"])
    gr = capi.Graph(tm2.write_tm2(g), keep_tensors=True)
    gr.set_input(x)
    gr.run()
    act = [i for i, t in enumerate(g.tensors) if t.name == "act"][0]
    with pytest.raises(capi.TamdError, match="fused"):
        gr.read_tensor(act)
    gr.close()


@pytest.mark.parametrize("case,kw,names_want", [
    ("negative_slope", dict(slope=-0.1), ["relu_i8", "pool_i8"]),         # not monotone: max and the map do not commute
    ("average_pool", dict(alg=1), ["relu_i8", "pool_i8"]),
    ("global_pool", dict(glob=1), ["relu_i8", "pool_i8"]),
    ("second_consumer", dict(second_consumer=True), ["relu_i8", "pool_i8"]),
])
def test_what_must_not_fuse_stays_two_launches_and_is_correct(ref, case, kw, names_want):
    dims, k, s, p, caffe = RELU_POOL_SHAPES["k2s2"]
    slope, s_in, s_relu, s_pool = RELU_POOL_SCALES["leaky0.1"]
    slope = kw.pop("slope", slope)
    g, x = relu_pool_graph(23, dims, k, s, p, caffe, slope, s_in, s_relu, s_pool, **kw)
    want = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8, 1)
    got, names = device(g, x)
    assert names == names_want, names
    same(want, got)


def test_relu_pool_into_a_concat_view(ref):
    g, x = relu_pool_concat_graph(31)
    want = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8, 1)
    got, names = device(g, x)
    assert names.count("relu_pool_i8") == 1 and "concat_copy_i8" not in names and "pool_i8" not in names, names
    same(want, got)


# ---- the whole graph -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yolo64(ref):
    """int8 YOLOv3-tiny at 64 x 64, batch 2: tmfile bytes, input, the reference's two outputs -- computed once, never changed"""
    g = models.build("yolov3_tiny", "int8", 2, res=64)
    x = models.synth_input(g, 3)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_INT8, 8)
    assert [w.shape for w in want] == [(2, 255, 2, 2), (2, 255, 4, 4)]
    for w in want:
        w.setflags(write=False)
    return b, x, want


@pytest.mark.parametrize("direct", [False, True], ids=["hipgraph", "direct_dispatch"])
def test_whole_int8_yolov3_tiny_equals_the_reference(yolo64, direct):
    b, x, want = yolo64
    gr = capi.Graph(b, direct_dispatch=direct)
    gr.set_input(x)
    first = gr.run()
    second = gr.run()
    if direct:
        assert gr.direct_packets() > 0
    else:
        names = [k["kernel"] for k in gr.profile(1)]
        # eleven leaky ReLUs: five feed a max-pool alone (one launch each), leaky4 feeds maxpool4 AND the route (two launches)
        assert names.count("upsample_i8") == 1 and names.count("relu_pool_i8") == 5 and names.count("relu_i8") == 6, names
        assert names.count("pool_i8") == 1, names
    gr.close()
    same(want, first)
    same(want, second)


def test_whole_int8_yolov3_tiny_through_the_plugin_is_one_subgraph(ref, yolo64):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    b, x, want = yolo64
    rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = tp.placement(rg)
    got = rg.outputs()
    rg.close()
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert len(real) == 1 and real[0][0] == "HIP", pl
    same(want, got)


def test_int8_yolov3_tiny_416_equals_the_committed_golden():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "yolov3_tiny_int8_416_seed3.npz"))
    g = models.build("yolov3_tiny", "int8", 1)
    x = models.synth_input(g, 3)
    got, names = device(g, x)
    same([gold["out0"], gold["out1"]], got)
    assert names.count("upsample_i8") == 1 and names.count("relu_pool_i8") == 5 and "concat_copy_i8" in names, names
