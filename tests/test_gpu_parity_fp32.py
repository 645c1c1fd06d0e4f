"""GPU parity, fp32: the HIP backend through the C ABI against the CPU oracle (double-accumulated
restatement: tests/test_fp32_oracle.py pins it to the real reference, whose own Winograd path carries most of THAT test's
budget).  Tolerance, written here: ABSOLUTE, max |device - oracle| <= 1e-4 (north_star: "fp32 within 1e-4"; the reference's own
conformance bar is absolute too, tests/op/test_onnx_op.h:173-188) -- every tensor in these tests is O(1..20), where binary32
accumulation sits around 1e-6.  The max |d| of every comparison is printed (pytest -s / the captured log)."""
import numpy as np
import pytest

from oracle import oracle
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_FP32, Graph

pytestmark = pytest.mark.gpu
ATOL = 1e-4


def close(got, want, what=""):
    d = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(want) else 0.0
    print("fp32 parity %s: max |d| = %.3g (|ref| max %.3g)" % (what, d, float(np.abs(want).max()) if np.size(want) else 0.0))
    return d <= ATOL


def run_hip(g, x):
    gr = capi.Graph(tm2.write_tm2(g))
    gr.set_input(x)
    out = gr.run()
    gr.close()
    return out


def conv_graph_f32(seed, n, cin, h, w, cout, k, s=1, p=0, group=1, act=0, bias=True, dil=1, geom=None):
    """`geom`: per-axis geometry (helpers.conv_geom) in place of k / s / p / dil"""
    from helpers import conv_geom, geom_out, geom_params
    rng = np.random.default_rng(seed)
    G = conv_geom(geom, k, s, p, dil)
    g = Graph(name="conv_f32_case")
    x = g.add_input("data", [n, cin, h, w], DT_FP32, None, None)
    fan = (cin // group) * G["kh"] * G["kw"]
    ins = [x, g.add_const("w", rng.normal(0, np.sqrt(2.0 / fan), size=(cout, cin // group, G["kh"], G["kw"])).astype(np.float32), DT_FP32, None, None)]
    if bias:
        ins.append(g.add_const("b", rng.uniform(-0.1, 0.1, size=(cout,)).astype(np.float32), DT_FP32, None, None))
    oh, ow = geom_out(h, w, G)
    y = g.add_tensor("out", [n, cout, oh, ow], DT_FP32, tm2.TT_VAR, None, None, None)
    ni = g.add_node("conv", "Convolution", ins, [y], input_channel=cin, output_channel=cout, group=group, activation=act, **geom_params(G))
    g.output_nodes = [ni]
    return g, rng.normal(0, 1, size=(n, cin, h, w)).astype(np.float32)


def pool_graph_f32(seed, n, c, h, w, alg, caffe, geom):
    """one fp32 Pooling node of per-axis geometry `geom` (helpers.pool_geom)"""
    from helpers import pool_geom, pool_geom_out, pool_geom_params
    rng = np.random.default_rng(seed)
    G = pool_geom(geom)
    g = Graph(name="pool_f32_case")
    x = g.add_input("data", [n, c, h, w], DT_FP32, None, None)
    oh, ow = pool_geom_out(h, w, G, 0, caffe)
    y = g.add_tensor("out", [n, c, oh, ow], DT_FP32, tm2.TT_VAR, None, None, None)
    g.output_nodes = [g.add_node("pool", "Pooling", [x], [y], alg=alg, **{"global": 0}, caffe_flavor=caffe, **pool_geom_params(G))]
    return g, rng.normal(0, 1, size=(n, c, h, w)).astype(np.float32)


F32_CONV = [
    (1, 3, 64, 64, 16, 3, 2, 1, 1, 0, True, 1),
    (2, 64, 20, 20, 128, 3, 1, 1, 1, 0, True, 1),
    (1, 128, 13, 13, 255, 1, 1, 0, 1, -1, True, 1),
    (1, 256, 13, 13, 512, 3, 1, 1, 1, 6, False, 1),
    (3, 7, 9, 11, 13, 3, 1, 1, 1, -1, True, 1),
    (1, 32, 12, 12, 16, 3, 1, 2, 1, 0, True, 2),
    (4, 64, 1, 1, 10, 1, 1, 0, 1, -1, True, 1),
    (1, 32, 12, 12, 32, 3, 1, 1, 32, 0, True, 1),
    (2, 24, 13, 13, 24, 3, 2, 1, 24, 6, True, 1),
]


@pytest.mark.parametrize("case", F32_CONV, ids=[str(c) for c in F32_CONV])
def test_conv_f32(case):
    n, cin, h, w, cout, k, s, p, group, act, bias, dil = case
    g, x = conv_graph_f32(3 + cin + cout, n, cin, h, w, cout, k, s, p, group, act, bias, dil)
    want = oracle.run_graph(g, x)[0]
    got = run_hip(g, x)[0].reshape(want.shape)
    assert got.dtype == np.float32
    assert close(got, want), "max |d| %g" % np.abs(got - want).max()


@pytest.mark.parametrize("name,batch", [("squeezenet_v1.1", 1), ("squeezenet_v1.1", 4), ("mobilenet_v1", 2)])
def test_fp32_models(name, batch):
    """BASELINE configs[0] (SqueezeNet-v1.1 fp32 227x227: conv / fire concat / max+avg pool / dropout / softmax) and
    MobileNet-v1 fp32 (depthwise)."""
    g = models.build(name, "fp32", batch)
    x = models.synth_input(g, 5, DT_FP32)
    want = oracle.run_graph(g, x)
    got = run_hip(g, x)
    for w, o in zip(want, got):
        assert close(o.reshape(w.shape), w, "%s b%d" % (name, batch)), "max |d| %g" % np.abs(o.reshape(w.shape) - w).max()
        assert np.abs(w).max() > 1e-3


@pytest.mark.parametrize("case", ["ssd_three_maps_concat", "non_square_fractional_sizes_clip", "no_flip_own_step_and_image"])
def test_priorbox_fp32_exact(case):
    """PriorBox in an fp32 graph: evaluated at prerun with the reference's own operations -> EXACT floats (== oracle == golden of
    the real reference), not merely 1e-4"""
    import os
    from helpers import PRIORBOX_CASES, priorbox_graph
    g, x = priorbox_graph(dtype=DT_FP32, **PRIORBOX_CASES[case])
    want = oracle.run_graph(g, x)[0]
    got = run_hip(g, x)[0].reshape(want.shape)
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.load(os.path.join(os.path.dirname(__file__), "golden", "priorbox_cases.npz"))["%s_fp32" % case])


@pytest.mark.parametrize("dims,axis", [([1, 5, 6, 7], 2), ([2, 3, 4, 9], 3), ([2, 8, 5], -1)])
def test_concat_any_axis_fp32(dims, axis):
    from helpers import axis_concat_graph
    g, x = axis_concat_graph(31 + axis, DT_FP32, dims, axis)
    want = oracle.run_graph(g, x)[0]
    got = run_hip(g, x)[0].reshape(want.shape)
    assert np.array_equal(got, want)       # leaky ReLU + copies: no rounding differences possible


# ---- Winograd F(2,3) (the reference's CPU backend: conv/x86/wino_conv_kernel_x86.c, F(4,3)) -------------------
WINO = [
    # n, cin, h, w, cout, pad, act, bias
    (1, 16, 8, 8, 64, 1, -1, True),
    (2, 64, 20, 20, 128, 1, 0, True),
    (3, 7, 9, 11, 13, 1, -1, True),          # odd maps (ragged last tile row / column), channels below every padding unit
    (1, 33, 15, 14, 70, 0, 6, False),        # pad 0, relu6, no bias
    (1, 256, 13, 13, 512, 1, 0, True),
    (4, 32, 56, 56, 32, 1, 0, True),         # tiles of several images in one GEMM column block
]


@pytest.mark.parametrize("case", WINO, ids=[str(c) for c in WINO])
def test_conv_f32_winograd_forced(case, monkeypatch):
    n, cin, h, w, cout, p, act, bias = case
    g, x = conv_graph_f32(11 + cin + cout, n, cin, h, w, cout, 3, 1, p, 1, act, bias, 1)
    want = oracle.run_graph(g, x)[0]
    monkeypatch.setenv("TAMD_F32_WINOGRAD", "1")
    gr = capi.Graph(tm2.write_tm2(g))
    gr.set_input(x)
    got = gr.run()[0].reshape(want.shape)
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    assert names == ["wino_in_f32", "wino_gemm_f32<F(2,3)>", "wino_out_f32"], names
    assert close(got, want), "max |d| %g" % np.abs(got - want).max()
    monkeypatch.setenv("TAMD_F32_WINOGRAD", "0")
    direct = run_hip(g, x)[0].reshape(want.shape)
    assert np.abs(direct - got).max() <= 2e-4 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("mode", ["0", "1"])
def test_squeezenet_fp32_winograd_modes(mode, monkeypatch):
    """the fire modules' expand3x3 convolutions write into the concat at a channel offset: both forms of the 3x3 land there"""
    monkeypatch.setenv("TAMD_F32_WINOGRAD", mode)
    g = models.build("squeezenet_v1.1", "fp32", 2)
    x = models.synth_input(g, 5, DT_FP32)
    want = oracle.run_graph(g, x)
    gr = capi.Graph(tm2.write_tm2(g))
    gr.set_input(x)
    got = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    assert any(k.startswith("wino_gemm") for k in names) == (mode == "1"), names
    for w_, o in zip(want, got):
        assert close(o.reshape(w_.shape), w_), "max |d| %g" % np.abs(o.reshape(w_.shape) - w_).max()


# ---- the single-hop bar: device against the REAL reference, absolute 1e-4 -----------------------------------
# The tests above go device -> oracle (double accumulation) at 1e-4 absolute, and tests/test_fp32_oracle.py goes oracle -> reference
# at 1e-4 + 1e-4 |ref| (the reference's own F(4,3) Winograd carries most of that budget): chained, that is looser than north_star's
# "fp32 within 1e-4".  Here the device's results (F(2,3) forced AND the direct form) meet the reference's own CPU results directly.
REF_SINGLE_HOP = [
    # n, cin, h, w, cout, k, s, p, group, act, bias        (3x3 / s1 cases with cin, cout >= 16, cout % 16 == 0, maps > 10: the
    (2, 64, 20, 20, 128, 3, 1, 1, 1, 0, True),             #  reference runs ITS Winograd F(4,3) there, winograd_support :1896-1915)
    (1, 256, 13, 13, 512, 3, 1, 1, 1, 0, True),
    (4, 32, 56, 56, 32, 3, 1, 1, 1, 0, True),
    (1, 16, 30, 30, 64, 3, 1, 1, 1, -1, True),             # SqueezeNet's expand3x3 shapes
    (1, 64, 14, 14, 256, 3, 1, 1, 1, 0, True),
    (1, 128, 13, 13, 255, 1, 1, 0, 1, -1, True),           # sgemm_fp32 cases
    (1, 3, 64, 64, 16, 3, 2, 1, 1, 0, True),
    (2, 24, 13, 13, 24, 3, 2, 1, 24, 6, True),             # depthwise
]


@pytest.mark.parametrize("wino", ["0", "1"], ids=["direct", "winograd_f23"])
@pytest.mark.parametrize("case", REF_SINGLE_HOP, ids=[str(c) for c in REF_SINGLE_HOP])
def test_conv_f32_against_the_real_reference_single_hop(case, wino, monkeypatch):
    from oracle import ref_capi
    if not ref_capi.available():
        pytest.skip("oracle/_ref/libtengine-lite.so not built")
    n, cin, h, w, cout, k, s, p, group, act, bias = case
    g, x = conv_graph_f32(100 + cin + cout + k, n, cin, h, w, cout, k, s, p, group, act, bias, 1)
    want = np.asarray(ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 4)[0])
    monkeypatch.setenv("TAMD_F32_WINOGRAD", wino)
    got = run_hip(g, x)[0].reshape(want.shape)
    assert close(got, want, "device (%s) vs the real reference %s" % ("F(2,3)" if wino == "1" else "direct", case)), "max |d| %g" % np.abs(got - want).max()


def test_squeezenet_fp32_against_the_real_reference_single_hop():
    """BASELINE configs[0] itself: every output of SqueezeNet-v1.1 on the device within 1e-4 ABSOLUTE of the reference CPU backend's"""
    from oracle import ref_capi
    if not ref_capi.available():
        pytest.skip("oracle/_ref/libtengine-lite.so not built")
    g = models.build("squeezenet_v1.1", "fp32", 1)
    x = models.synth_input(g, 5, DT_FP32)
    want = ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 4)
    got = run_hip(g, x)
    for w_, o in zip(want, got):
        assert close(o.reshape(np.asarray(w_).shape), np.asarray(w_), "squeezenet_v1.1 vs the real reference")
