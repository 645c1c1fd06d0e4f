"""The bandwidth kernels of f32_kernels.hip -- upsample_f32, relu_f32 (ReLU, leaky ReLU, the ReLU6 node), eltwise_f32, softmax_f32,
pool_f32 -- on the device against oracle.run_graph.  Where the operation moves or clamps values, or is ONE correctly rounded operation
(a leaky ReLU's product, an Eltwise), the floats must be equal; sums and exponentials meet test_gpu_parity_fp32.py's ATOL (1e-4 absolute).
upsample_f32 and the ReLU6 node meet a reference here for the first time: tests/test_fp32_oracle.py pins the oracle's statement of both to
the real reference.  Shapes are the smallest that leave a plane ragged against the 256-lane block, need more than one block per plane, or
put the output at a channel offset of a wider image (written in place into a Concat behind another input)."""
import numpy as np
import pytest

from helpers import f32_unary_graph, pool_geom, pool_geom_out, pool_geom_params
from oracle import oracle
from tengine_amd import tm2
from tengine_amd.tm2 import DT_FP32, Graph
from test_gpu_geometry import device
from test_gpu_parity_fp32 import close

pytestmark = pytest.mark.gpu


def run_both(g, x, launches, what):
    """-> (device outputs shaped as the oracle's, the oracle's); the launch list is `launches`"""
    wants = oracle.run_graph(g, x)
    outs, names = device(tm2.write_tm2(g), x)
    assert names == launches, (what, names)
    assert len(outs) == len(wants)
    return [o.reshape(w.shape) for o, w in zip(outs, wants)], wants


def same(got, want, what):
    bad = np.argwhere(got != want)
    print("fp32 glue %s: %d of %d floats differ" % (what, len(bad), want.size))
    assert got.dtype == np.float32 and len(bad) == 0, "%s: %d of %d floats differ from the oracle, first at %s: %r != %r" % (
        what, len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def var(g, name, dims):
    return g.add_tensor(name, list(dims), DT_FP32, tm2.TT_VAR, None, None, None)


def behind_another_input(op, dims, out_dims=None, **params):
    """data -> [Upsample, where `op` changes the map size ->] leaky ReLU r; data -> `op` -> y; Concat([r, y]).  r and y are both written
    in place, y at out_c0 = C of an image of 2 C channels: no concat_f32 launch.  -> (graph, names of the launches in front of `op`'s)"""
    g = Graph(name="f32_%s_slice_case" % op)
    x = g.add_input("data", list(dims), DT_FP32, None, None)
    out_dims = list(out_dims or dims)
    front, src = [], x
    if out_dims != list(dims):
        src = var(g, "a", out_dims)
        g.add_node("up_a", "Upsample", [x], [src], scale=params["scale"])
        front.append("upsample_f32")
    r = var(g, "r", out_dims)
    g.add_node("leaky", "ReLU", [src], [r], negative_slope=0.25)
    front.append("relu_f32")
    y = var(g, "y", out_dims)
    g.add_node(op.lower(), op, [x], [y], **params)
    cat = var(g, "cat", [out_dims[0], 2 * out_dims[1]] + out_dims[2:])
    g.output_nodes = [g.add_node("cat", "Concat", [r, y], [cat], axis=1)]
    return g, front


# ---- upsample_f32 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sliced", [False, True], ids=["standalone", "concat_slice"])
@pytest.mark.parametrize("dims", [(2, 5, 3, 5), (1, 3, 17, 19)], ids=["2x5x3x5", "1x3x17x19"])        # the second: several blocks per plane
@pytest.mark.parametrize("scale", [2, 3])
def test_upsample_f32(scale, dims, sliced):
    n, c, h, w = dims
    od = [n, c, h * scale, w * scale]
    x = np.random.default_rng(8000 + scale + h).normal(0, 1, size=dims).astype(np.float32)
    if sliced:
        g, front = behind_another_input("Upsample", dims, od, scale=scale)
        launches = front + ["upsample_f32"]
    else:
        g, launches = f32_unary_graph("Upsample", dims, od, scale=scale), ["upsample_f32"]
    (got,), (want,) = run_both(g, x, launches, "upsample")
    same(got, want, "upsample x%d %s %s" % (scale, dims, "into a Concat slice" if sliced else "standalone"))
    assert len(np.unique(want[:, -c:])) == x.size          # every input element is somewhere in the output: a wrong source index shows


# ---- relu_f32 ----------------------------------------------------------------------------------------------------------------------------
RELU = {"relu": ("ReLU", dict(negative_slope=0.0)), "leaky": ("ReLU", dict(negative_slope=0.1)), "relu6": ("ReLU6", {})}


@pytest.mark.parametrize("sliced", [False, True], ids=["standalone", "concat_slice"])
@pytest.mark.parametrize("kind", sorted(RELU))
def test_relu_f32(kind, sliced):
    """x spans below 0 and above 6, the clamps themselves among the values"""
    op, params = RELU[kind]
    dims = (2, 7, 5, 9)
    x = np.random.default_rng(8100 + len(kind)).uniform(-4, 10, size=dims).astype(np.float32)
    x.ravel()[:4] = [0.0, 6.0, np.nextafter(np.float32(6), np.float32(7)), -1e-30]
    if sliced:
        g, front = behind_another_input(op, dims, **params)
        launches = front + ["relu_f32"]
    else:
        g, launches = f32_unary_graph(op, dims, **params), ["relu_f32"]
    (got,), (want,) = run_both(g, x, launches, kind)
    same(got, want, "%s %s" % (kind, "into a Concat slice" if sliced else "standalone"))
    y = want[:, -dims[1]:]
    assert y.max() == (6 if kind == "relu6" else x.max()) and y.min() == (0 if kind != "leaky" else np.float32(0.1) * x.min())


# ---- eltwise_f32 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("etype", ["ELT_PROD", "ELT_SUM", "ELT_SUB", "ELT_MAX"])
def test_eltwise_f32(etype):
    """546 elements (two full blocks and a ragged third); the operands come from two different producers -- a leaky ReLU and a ReLU6 of
    the input -- so that a swap of the two shows in SUB"""
    dims = (2, 3, 7, 13)
    g = Graph(name="f32_eltwise_case")
    x = g.add_input("data", list(dims), DT_FP32, None, None)
    a, b, y = var(g, "a", dims), var(g, "b", dims), var(g, "out", dims)
    g.add_node("leaky", "ReLU", [x], [a], negative_slope=0.1)
    g.add_node("relu6", "ReLU6", [x], [b])
    g.output_nodes = [g.add_node("elt", "Eltwise", [a, b], [y], type=getattr(tm2, etype), caffe_flavor=1)]
    xin = np.random.default_rng(8200).normal(0, 4, size=dims).astype(np.float32)
    (got,), (want,) = run_both(g, xin, ["relu_f32", "relu_f32", "eltwise_f32"], etype)
    same(got, want, etype)
    if etype == "ELT_SUB":
        assert np.count_nonzero(want) > want.size // 2 and not np.array_equal(want, -want)


# ---- softmax_f32 -------------------------------------------------------------------------------------------------------------------------
SOFTMAX = {
    "axis1_of_2x21x5x7": ((2, 21, 5, 7), 1, 0.0, 1.0),
    "axis2_of_3x40x21": ((3, 40, 21), 2, 0.0, 1.0),
    "last_axis_of_4x100": ((4, 100), -1, 0.0, 1.0),
    "one_channel": ((2, 1, 3, 3), 1, 0.0, 1.0),
    "logits_near_90": ((2, 10, 4, 4), 1, 90.0, 3.0),           # exp(90) overflows binary32: only a softmax that subtracts the max survives
}


@pytest.mark.parametrize("name", sorted(SOFTMAX))
def test_softmax_f32(name):
    dims, axis, mean, std = SOFTMAX[name]
    x = (np.random.default_rng(8300 + len(name)).normal(0, std, size=dims) + mean).astype(np.float32)
    g = f32_unary_graph("Softmax", dims, axis=axis)
    (got,), (want,) = run_both(g, x, ["softmax_f32"], name)
    assert np.isfinite(got).all() and close(got, want, "softmax %s" % name), np.abs(got - want).max()
    sums = got.astype(np.float64).sum(axis=axis)
    print("softmax %s: max |row sum - 1| = %.3g" % (name, np.abs(sums - 1).max()))
    assert np.abs(sums - 1).max() <= 1e-5
    assert np.array_equal(got.argmax(axis=axis), want.argmax(axis=axis))


# ---- pool_f32 ----------------------------------------------------------------------------------------------------------------------------
def pool_f32(x, alg, caffe=0, glob=0, **geom):
    """one Pooling node on x -> (device output, oracle output); every window of every case here overlaps the image"""
    n, c, h, w = x.shape
    G = pool_geom(geom)
    oh, ow = pool_geom_out(h, w, G, glob, caffe)
    for o, k, s, p, size in ((oh, G["kh"], G["sh"], G["ph0"], h), (ow, G["kw"], G["sw"], G["pw0"], w)):
        assert glob or ((o - 1) * s - p < size and k - p > 0), "a window lies wholly in the padding"
    g = f32_unary_graph("Pooling", x.shape, [n, c, oh, ow], alg=alg, **{"global": glob}, caffe_flavor=caffe, **pool_geom_params(G))
    (got,), (want,) = run_both(g, x, ["pool_f32"], "pool")
    return got, want


@pytest.mark.parametrize("hw", [7, 1])
def test_pool_f32_global_average(hw):
    x = np.random.default_rng(8400 + hw).normal(0, 1, size=(2, 5, hw, hw)).astype(np.float32)
    got, want = pool_f32(x, 1, glob=1, kh=hw, kw=hw)
    assert want.shape == (2, 5, 1, 1) and close(got, want, "global average %dx%d" % (hw, hw))


S2P1 = dict(kh=3, kw=3, sh=2, sw=2, ph0=1, ph1=1, pw0=1, pw1=1)


def test_pool_f32_max_padding_is_not_a_value():
    """every input is <= -1: a max that took the padding for a 0 would show at the border"""
    x = (-1 - np.abs(np.random.default_rng(8410).normal(0, 1, size=(2, 3, 9, 11)))).astype(np.float32)
    got, want = pool_f32(x, 0, **S2P1)
    assert want.shape == (2, 3, 5, 6)
    same(got, want, "max 3x3 stride 2 pad 1")
    assert got.max() <= -1


def test_pool_f32_average_window_rule():
    """caffe_flavor 1 divides by the window clipped to the PADDED image, 0 by the window clipped to the image: on this 9x11 map every
    border output's window reaches into the padding (4 or 6 cells against 9, 6 against 9 at the far edges), no interior one's does"""
    x = (1 + np.abs(np.random.default_rng(8420).normal(0, 1, size=(2, 3, 9, 11)))).astype(np.float32)         # positive: no sum is 0
    got0, want0 = pool_f32(x, 1, caffe=0, **S2P1)
    got1, want1 = pool_f32(x, 1, caffe=1, **S2P1)
    assert want0.shape == want1.shape == (2, 3, 5, 6)
    assert close(got0, want0, "average 3x3 stride 2 pad 1, caffe_flavor 0") and close(got1, want1, "average 3x3 stride 2 pad 1, caffe_flavor 1")
    border = np.ones(want0.shape, bool)
    border[:, :, 1:-1, 1:-1] = False
    assert np.array_equal(got0[~border], got1[~border]) and np.all(got0[border] > got1[border] * 1.4)


@pytest.mark.parametrize("alg", [0, 1], ids=["max", "average"])
def test_pool_f32_kernel2_stride1_on_13x13(alg):
    x = np.random.default_rng(8430 + alg).normal(0, 1, size=(2, 3, 13, 13)).astype(np.float32)
    got, want = pool_f32(x, alg, kh=2, kw=2, sh=1, sw=1)
    assert want.shape == (2, 3, 12, 12)
    if alg == 0:
        same(got, want, "max 2x2 stride 1 on 13x13")
    else:
        assert close(got, want, "average 2x2 stride 1 on 13x13")
