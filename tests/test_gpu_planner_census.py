"""A census of the two NCHW planners (graph_u8.hip, graph_f32.hip): one small graph per node function and per convolution form, so that
every one of them plans at least once through append_steps (graph_plan_common.hip).  A node function that forgets to state what its
launch reads and writes fails prerun with "does not state what it reads and writes" in the case that names it; one that states a
write over its own read fails with "writes memory that it reads".  Every case: prerun succeeds, the launch list is the expected one,
the output meets the bar of the existing suites -- uint8 bytes == the oracle, the integer path at test_gpu_u8_int.py's bar, fp32 at
test_gpu_parity_fp32.py's ATOL.  Shapes: N = 2, 8 channels, 8 x 8 maps unless a kernel's own rule asks for more (conv_u8_pw: K = 32,
conv_u8_c3 and the patch kernel: 16 channels, conv_u8_rgb3x3: 3, the DMA form: K = 32400).  The byte-map planners that both
quantised graphs share (graph_plan_maps.hip: tables, PReLU, Interp, Split, ShuffleChannel) go through the same append_steps in
the uint8 cases of test_gpu_lut.py / _prelu.py / _interp.py / _shuffle.py, against the real reference's bytes."""
import numpy as np
import pytest

from geometry_cases import P
from helpers import (PRIORBOX_CASES, _u8q, priorbox_graph, u8_conv_graph, u8_conv_int_model, u8_conv_pool_graph, u8_fc_graph, u8_pool_graph,
                     u8_route_graph, u8_ssd_head_graph, u8_unary_graph)
from oracle import oracle
from slice_helpers import u8_concat_graph
from tengine_amd import tm2
from tengine_amd.tm2 import DT_FP32, DT_UINT8, Graph
from test_gpu_geometry import close, device, exact
from test_gpu_parity_fp32 import conv_graph_f32, pool_graph_f32

pytestmark = pytest.mark.gpu

NO_FORM = {"u8_patch": 0, "u8_pw": 0, "u8_c3": 0}          # the GEMM family alone


def glue_graph(dtype, seed=7, n=2, c=8, h=8, w=8):
    """data -> ReLU r (written in place into the Concat); data -> max-pool 2x2 -> Upsample x2 -> u; Eltwise SUM(u, data) -> e (copied into
    the Concat); Concat([r, e], channels) -> Softmax over the channels.  uint8: r carries the Concat's quantisation (the in-place rule).
    fp32: u is a leaky ReLU of data instead -- upsample_f32 is planned by the function that plans relu_f32 (plan_map_f32) and is compared
    with the oracle in test_gpu_f32_glue.py; pool_f32 has a case of its own"""
    rng = np.random.default_rng(seed)
    u8 = dtype == DT_UINT8
    g = Graph(name="glue_case")
    q = lambda: _u8q(rng) if u8 else (None, None)
    wrap = lambda s, z: ([s], [z]) if u8 else (None, None)
    var = lambda name, dims, sz: g.add_tensor(name, dims, dtype, tm2.TT_VAR, None, *wrap(*sz))
    x = g.add_input("data", [n, c, h, w], dtype, *wrap(*q()))
    cq = q()
    r = var("r", [n, c, h, w], cq)
    g.add_node("relu", "ReLU", [x], [r], negative_slope=0.0)
    if u8:
        p = var("p", [n, c, h // 2, w // 2], q())
        g.add_node("pool", "Pooling", [x], [p], alg=0, kernel_h=2, kernel_w=2, stride_h=2, stride_w=2, **{"global": 0}, caffe_flavor=0, pad_h0=0, pad_w0=0,
                   pad_h1=0, pad_w1=0)
        u = var("u", [n, c, h, w], q())
        g.add_node("up", "Upsample", [p], [u], scale=2)
    else:
        u = var("u", [n, c, h, w], q())
        g.add_node("leaky", "ReLU", [x], [u], negative_slope=0.1)
    e = var("e", [n, c, h, w], q())
    g.add_node("sum", "Eltwise", [u, x], [e], type=tm2.ELT_SUM, caffe_flavor=1)
    cat = var("cat", [n, 2 * c, h, w], cq)
    g.add_node("cat", "Concat", [r, e], [cat], axis=1)
    sm = var("prob", [n, 2 * c, h, w], (1.0 / 256, 0) if u8 else (None, None))
    g.output_nodes = [g.add_node("prob", "Softmax", [cat], [sm], axis=1)]
    xin = rng.integers(0, 256, size=(n, c, h, w)).astype(np.uint8) if u8 else rng.normal(0, 1, size=(n, c, h, w)).astype(np.float32)
    return g, xin


def fc_graph_f32(seed, n, hidden_dims, nout):
    rng = np.random.default_rng(seed)
    g = Graph(name="fc_f32_case")
    hidden = int(np.prod(hidden_dims))
    x = g.add_input("data", [n] + list(hidden_dims), DT_FP32, None, None)
    ins = [x, g.add_const("w", rng.normal(0, np.sqrt(2.0 / hidden), size=(nout, hidden)).astype(np.float32), DT_FP32, None, None),
           g.add_const("b", rng.uniform(-0.1, 0.1, size=(nout,)).astype(np.float32), DT_FP32, None, None)]
    y = g.add_tensor("out", [n, nout], DT_FP32, tm2.TT_VAR, None, None, None)
    g.output_nodes = [g.add_node("fc", "FullyConnected", ins, [y], num_output=nout)]
    return g, rng.normal(0, 1, size=[n] + list(hidden_dims)).astype(np.float32)


# name -> (graph builder, pins, environment, graph options, the launch list as profile() shows it, the bar).  priorbox_concat_once: the
# Concat of PriorBox outputs is launched once at prerun (Step::once) and is no launch of a pass; it still goes through append_steps
U8 = {
    "conv_gemm": (lambda: u8_conv_graph(11, 2, 8, 8, 8, 8, 3, 1, 1), NO_FORM, {}, {}, ["conv_u8_mfma_16x64"], "bytes"),
    "conv_lanes_default": (lambda: u8_conv_graph(11, 2, 8, 8, 8, 8, 3, 1, 1), {}, {}, {}, ["conv_u8_lanes<3x3>"], "bytes"),
    "conv_patch": (lambda: u8_conv_graph(12, 2, 16, 8, 8, 8, 3, 1, 1), {"u8_patch": 1, "u8_patch_cfg": 0}, {}, {}, ["conv_u8_patch_64x64<3x3>"], "bytes"),
    "conv_pw": (lambda: u8_conv_graph(13, 2, 32, 8, 8, 8, 1), {"u8_patch": 0, "u8_pw": 1}, {}, {}, ["conv_u8_pw<k32>"], "bytes"),
    "conv_c3": (lambda: u8_conv_graph(14, 2, 16, 8, 8, 8, 3, 1, 1), {"u8_patch": 0, "u8_c3": 1}, {}, {}, ["conv_u8_c3<c16>"], "bytes"),
    "conv_rgb3x3": (lambda: u8_conv_graph(15, 2, 3, 8, 8, 8, 3, 1, 1), {"u8_rgb3x3": 1}, {}, {}, ["conv_u8_rgb3x3"], "bytes"),
    "conv_direct": (lambda: u8_conv_graph(16, 2, 8, 8, 8, 8, 3, 1, 1, group=8), {}, {}, {}, ["conv_u8_direct"], "bytes"),
    "conv_integer": (lambda: u8_conv_graph(17, 2, 8, 8, 8, 8, 3, 1, 1), {}, {}, {"u8_integer": True}, ["conv_u8i_32x256"], "integer"),
    "conv_integer_first": (lambda: u8_conv_graph(18, 2, 3, 8, 8, 8, 3, 1, 1), {}, {}, {"u8_integer": True}, ["conv_u8i_rgb3x3"], "integer"),
    "conv_dma": (lambda: u8_conv_graph(2000 + 3600 + 8 + 3, 1, 3600, 3, 3, 8, 3, 1, 1), {}, {}, {}, ["dequant_u8_f32", "conv_f32_mfma_16x64"], "bytes"),
    "conv_relu_pool": (lambda: u8_conv_pool_graph(19, 2, 8, 8, 8, 8), NO_FORM, {}, {}, ["conv_u8_mfma_16x64+relu+maxpool"], "bytes"),
    "conv_into_concat_slice": (lambda: u8_concat_graph(20, 8, 3, 8, True), NO_FORM, {}, {}, ["conv_u8_mfma_16x64", "conv_u8_mfma_16x64"], "bytes"),
    "fc": (lambda: u8_fc_graph(21, 2, [8, 8, 8], 8), {}, {}, {}, ["fc_u8"], "bytes"),
    "softmax": (lambda: u8_unary_graph(22, "Softmax", [2, 8, 8, 8], axis=1), {}, {}, {}, ["softmax_u8"], "bytes"),
    "pool": (lambda: u8_pool_graph(23, 2, 8, 8, 8, 0, 2, 2), {}, {}, {}, ["pool_u8"], "bytes"),
    "relu_pool_upsample_concat": (lambda: u8_route_graph(24, 2, 8, 4, 4), {}, {}, {}, ["relu_u8", "pool_u8", "upsample_u8", "concat_u8<x2>"], "bytes"),
    "glue": (lambda: glue_graph(DT_UINT8), {}, {}, {}, ["relu_u8", "pool_u8", "upsample_u8", "eltwise_u8", "concat_u8", "softmax_u8"], "bytes"),
    "ssd_heads_permute_concat": (lambda: u8_ssd_head_graph(25, 2, 8, 8, 8), NO_FORM, {}, {},
                                 ["pool_u8", "conv_u8_mfma_16x64", "conv_u8_mfma_32x64", "permute_concat_u8<x2>"], "bytes"),
    "permute": (lambda: u8_ssd_head_graph(26, 2, 8, 8, 8, standalone_permute=True), NO_FORM, {}, {}, ["pool_u8", "conv_u8_mfma_16x64", "permute_u8"], "bytes"),
    "priorbox_concat_once": (lambda: priorbox_graph(dtype=DT_UINT8, **PRIORBOX_CASES["no_flip_own_step_and_image"]), {}, {}, {},
                             ["pool_u8", "pool_u8"], "bytes"),
}
F32 = {
    "conv_direct_form": (lambda: conv_graph_f32(31, 2, 8, 8, 8, 8, 3, 1, 1), {}, {"TAMD_F32_WINOGRAD": 0}, {}, ["conv_f32_mfma_16x64"], "fp32"),
    "conv_winograd": (lambda: conv_graph_f32(31, 2, 8, 8, 8, 8, 3, 1, 1), {}, {"TAMD_F32_WINOGRAD": 1}, {},
                      ["wino_in_f32", "wino_gemm_f32<F(2,3)>", "wino_out_f32"], "fp32"),
    "conv_grouped": (lambda: conv_graph_f32(32, 2, 8, 8, 8, 8, 3, 1, 1, group=4), {}, {}, {}, ["conv_f32_direct"], "fp32"),
    "fc": (lambda: fc_graph_f32(33, 2, [8, 8, 8], 8), {}, {}, {}, ["conv_f32_mfma_16x64"], "fp32"),
    "pool": (lambda: pool_graph_f32(34, 2, 8, 8, 8, 0, 0, P((2, 2), (2, 2), (0, 0, 0, 0))), {}, {}, {}, ["pool_f32"], "fp32"),
    "glue": (lambda: glue_graph(DT_FP32), {}, {}, {}, ["relu_f32", "relu_f32", "eltwise_f32", "concat_f32", "softmax_f32"], "fp32"),
    "priorbox_concat_once": (lambda: priorbox_graph(dtype=DT_FP32, **PRIORBOX_CASES["no_flip_own_step_and_image"]), {}, {}, {},
                             ["pool_f32", "pool_f32"], "fp32"),
}


def census(table, name):
    build, pins, env, kw, expected, bar = table[name]
    g, x = build()
    wants = oracle.run_graph(g, x)
    outs, names = device(tm2.write_tm2(g), x, pins=pins, env=env, **kw)          # (a failed prerun raises here, with the library's message)
    print("census %s: %s" % (name, names))
    assert names == expected, (name, names)
    assert len(outs) == len(wants)
    for got, want in zip(outs, wants):
        if bar == "fp32":
            close(got, want, name)
        elif bar == "integer":       # test_gpu_u8_int.py's bar: the integer formula's model byte for byte, the reference within one step
            model = u8_conv_int_model(g, x)
            assert np.array_equal(got.reshape(model.shape), model), name
            d = np.abs(model.astype(int) - want.astype(int))
            print("census %s: max |d| %d, %d of %d differ from the reference" % (name, d.max(), np.count_nonzero(d), d.size))
            assert d.max() <= 1 and np.count_nonzero(d) / d.size < 2e-3, name
        else:
            exact(got, want, name)


@pytest.mark.parametrize("name", sorted(U8))
def test_uint8_planner_census(name):
    census(U8, name)


@pytest.mark.parametrize("name", sorted(F32))
def test_fp32_planner_census(name):
    census(F32, name)
