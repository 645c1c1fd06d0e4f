"""fp32 (parity bar 1e-4): the oracle's fp32 restatement (double accumulation) against the real
reference's fp32 kernels (im2col + sgemm, Winograd F(4,3) for the eligible 3x3 layers, direct depthwise)."""
import numpy as np
import pytest

from oracle import oracle, ref_capi
from tengine_amd import models, tm2

TOL = dict(rtol=1e-4, atol=1e-4)
needs_ref = pytest.mark.skipif(not ref_capi.available(), reason="reference library not built (oracle/build_ref.py)")


# anisotropic / asymmetric geometry (tests/geometry_cases.py): the tables the device runs in test_gpu_geometry.py, and the two 3x3 / s1
# shapes it forces through Winograd (the second is one the reference runs ITS Winograd F(4,3) on: its pads go through that code too)
from geometry_cases import ALL_CONV, F32_WINO, POOLS, seed_of  # noqa: E402
from test_gpu_parity_fp32 import conv_graph_f32, pool_graph_f32  # noqa: E402


def geometry_f32_conv(name):
    n, cin, h, w, cout, group, act, geom = (ALL_CONV.get(name) or F32_WINO[name])
    return conv_graph_f32(seed_of(name), n, cin, h, w, cout, 1, group=group, act=act, geom=geom)


@needs_ref
@pytest.mark.parametrize("name", sorted(ALL_CONV) + sorted(F32_WINO))
def test_conv_fp32_geometry_oracle_matches_reference(name):
    g, x = geometry_f32_conv(name)
    want = ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 2)[0]
    got = oracle.run_graph(g, x)[0]
    assert list(want.shape) == list(got.shape)
    assert np.allclose(want, got, **TOL), np.abs(want - got).max()
    assert np.abs(want).max() > 1e-3


@needs_ref
@pytest.mark.parametrize("name", sorted(POOLS))
def test_pool_fp32_geometry_oracle_matches_reference(name):
    n, c, h, w, alg, caffe, geom = POOLS[name]
    g, x = pool_graph_f32(seed_of(name), n, c, h, w, alg, caffe, geom)
    want = ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 2)[0]
    got = oracle.run_graph(g, x)[0]
    assert want.shape == got.shape and np.allclose(want, got, **TOL) and np.abs(want).max() > 1e-3


from helpers import f32_unary_graph as unary_graph_f32  # noqa: E402


@needs_ref
@pytest.mark.parametrize("scale", [2, 3])
def test_upsample_fp32_oracle_is_the_reference(scale):
    """upsample_ref.c moves values: the oracle's nearest repeat equals it float for float"""
    n, c, h, w = 2, 5, 3, 5
    g = unary_graph_f32("Upsample", [n, c, h, w], [n, c, h * scale, w * scale], scale=scale)
    x = np.random.default_rng(60 + scale).normal(0, 1, size=(n, c, h, w)).astype(np.float32)
    want = ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 2)[0]
    got = oracle.run_graph(g, x)[0]
    assert want.shape == got.shape == (n, c, h * scale, w * scale)
    assert np.array_equal(want, got) and len(np.unique(got)) == x.size


@needs_ref
def test_relu6_fp32_oracle_is_the_reference():
    """relu6_ref.c clamps: equal float for float, on inputs from below 0 to above 6 with the edges themselves among them.
    ref_relu6_fp32 loops over the channels of ONE image (relu6_ref.c:95-123 has no batch loop), so of the (2,8,9,9) run only image 0
    is the reference's statement; image 1 is held to it as an input of its own, and so is every value of the tensor."""
    x = np.random.default_rng(63).uniform(-3, 9, size=(2, 8, 9, 9)).astype(np.float32)
    x.ravel()[:6] = [0.0, -0.0, 6.0, np.nextafter(np.float32(6), np.float32(7)), np.nextafter(np.float32(6), np.float32(0)), -1e-30]
    x[1].ravel()[:3] = [6.0, 0.0, 1e30]
    assert x.min() < -2 and x.max() > 8 and ((x > 0) & (x < 6)).sum() > 100
    g = unary_graph_f32("ReLU6", x.shape)
    got = oracle.run_graph(g, x)[0]
    want = ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 2)[0]
    assert want.shape == got.shape and np.array_equal(want[0], got[0])
    g1 = unary_graph_f32("ReLU6", (1,) + x.shape[1:])
    for i in range(x.shape[0]):
        want_i = ref_capi.run_model(tm2.write_tm2(g1), x[i:i + 1], ref_capi.MODE_FP32, 2)[0]
        assert np.array_equal(want_i[0], got[i]), i
    assert got.min() == 0 and got.max() == 6 and np.array_equal(got, np.clip(x, 0, 6))


@needs_ref
@pytest.mark.parametrize("name", ["squeezenet_v1.1", "mobilenet_v1"])
def test_fp32_models_oracle_matches_reference(name):
    g = models.build(name, "fp32", 1)
    x = models.synth_input(g, 5, tm2.DT_FP32)
    want = ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_FP32, 4)
    got = oracle.run_graph(g, x)
    for w, o in zip(want, got):
        assert np.allclose(w, o.reshape(w.shape), **TOL)
        assert np.abs(w).max() > 1e-3
