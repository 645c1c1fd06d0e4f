"""Seeded int8 graphs around the YOLOv3-tiny pieces -- nearest Upsample (alone, and into a channel Concat) and ReLU -> max-pool --
for tests/test_gpu_int8_yolo.py (kept apart from the test file like helpers.py).  Everything is checked against the REAL reference (the `ref`
fixture): upsample_ref.c runs its uint8 routine on the int8 bytes, which no signed restatement reproduces."""
import numpy as np

from tengine_amd import tm2
from tengine_amd.tm2 import DT_INT8, DT_INT32, Graph


def _scales(rng, n, lo=0.002, hi=0.02):
    return [float(np.float32(v)) for v in rng.uniform(lo, hi, size=n)]


def all_bytes_inputs(seed, dims):
    """int8 inputs of shape `dims` that together hold every byte value -128 .. 127 (one input where the shape has 256 elements)"""
    rng = np.random.default_rng(seed)
    size = int(np.prod(dims))
    count = -(-256 // size)
    flat = np.concatenate([np.arange(-128, 128), rng.integers(-128, 128, size=count * size - 256)]).astype(np.int8)
    flat = flat[rng.permutation(flat.size)]
    xs = [flat[i * size:(i + 1) * size].reshape(dims) for i in range(count)]
    assert len(np.unique(np.concatenate([x.ravel() for x in xs]))) == 256
    return xs


def upsample_graph(dims, scale, s_in, s_out):
    g = Graph(name="i8_upsample_case")
    x = g.add_input("data", list(dims), DT_INT8, [float(np.float32(s_in))], [0])
    n, c, h, w = dims
    y = g.add_tensor("up", [n, c, h * scale, w * scale], DT_INT8, tm2.TT_VAR, None, [float(np.float32(s_out))], [0])
    g.output_nodes = [g.add_node("upsample", "Upsample", [x], [y], scale=float(scale))]
    return g


def _conv(g, rng, name, x, cin, cout, oh, ow, n, stride=1, out_scale=None):
    wq = rng.integers(-127, 128, size=(cout, cin, 1, 1)).astype(np.int8)
    ws = _scales(rng, cout)
    ins = [x, g.add_const(name + "_w", wq, DT_INT8, ws, [0] * cout),
           g.add_const(name + "_b", rng.integers(-2000, 2000, size=(cout,)).astype(np.int32), DT_INT32, [1.0], [0])]
    xs = g.tensors[x].scales[0]
    os_ = out_scale if out_scale is not None else float(np.float32(xs * np.mean(ws) * 73.0 * np.sqrt(cin) * 73.0 / 60.0))
    y = g.add_tensor(name, [n, cout, oh, ow], DT_INT8, tm2.TT_VAR, None, [os_], [0])
    g.add_node(name, "Convolution", ins, [y], kernel_h=1, kernel_w=1, stride_h=stride, stride_w=stride, dilation_h=1, dilation_w=1,
               input_channel=cin, output_channel=cout, group=1, activation=-1, pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
    return y


def upsample_concat_graph(seed, n=1, h=3, w=5, side=48, upsample_first=True, same_scale=True):
    """data [n, 16, 2h, 2w] -> conv(16 -> 32, 1x1, stride 2) -> ReLU 0.1 -> conv(32 -> 32, 1x1) -> Upsample x2   --\\
                            -> conv(16 -> `side`, 1x1), which carries the concat's scale (written in place)        --> Concat
    `same_scale`: the Upsample's output carries the concat's scale too (the quantiser's convention); otherwise its own."""
    rng = np.random.default_rng(seed)
    g = Graph(name="i8_upsample_concat_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    x = g.add_input("data", [n, 16, 2 * h, 2 * w], DT_INT8, [xs], [0])
    a = _conv(g, rng, "conv_a", x, 16, 32, h, w, n, stride=2)
    sa = g.tensors[a].scales[0]
    r = g.add_tensor("leaky", [n, 32, h, w], DT_INT8, tm2.TT_VAR, None, [float(np.float32(sa * 0.8))], [0])
    g.add_node("leaky", "ReLU", [a], [r], negative_slope=0.1)
    b = _conv(g, rng, "conv_b", r, 32, 32, h, w, n)
    sb = g.tensors[b].scales[0]
    cat_s = float(np.float32(sb * 1.31))
    u = g.add_tensor("up", [n, 32, 2 * h, 2 * w], DT_INT8, tm2.TT_VAR, None, [cat_s if same_scale else float(np.float32(sb * 0.77))], [0])
    g.add_node("upsample", "Upsample", [b], [u], scale=2.0)
    c = _conv(g, rng, "conv_side", x, 16, side, 2 * h, 2 * w, n, out_scale=cat_s)
    ins = [u, c] if upsample_first else [c, u]
    y = g.add_tensor("cat", [n, 32 + side, 2 * h, 2 * w], DT_INT8, tm2.TT_VAR, None, [cat_s], [0])
    g.output_nodes = [g.add_node("route", "Concat", ins, [y], axis=1)]
    return g, rng.integers(-127, 128, size=(n, 16, 2 * h, 2 * w)).astype(np.int8)


# (dims, kernel, stride, pad, caffe_flavor): the plain 2x2 / 2, YOLOv3-tiny's sixth pool (darknet flavour, total pad 1: 0 | 1, 'same'
# at stride 1) and a padded 3x3 / 2
RELU_POOL_SHAPES = {
    "k2s2": ([2, 5, 7, 5], 2, 2, 0, 0),
    "k2s1_same": ([1, 20, 6, 6], 2, 1, 1, 2),
    "k3s2p1": ([1, 4, 9, 9], 3, 2, 1, 0),
}
# (slope, input scale, ReLU output scale, pool output scale); the last: the quantiser's convention for a max-pool (scale shared)
RELU_POOL_SCALES = {
    "relu": (0.0, 0.021, 0.017, 0.024),
    "leaky0.1": (0.1, 0.02, 0.05, 0.031),
    "leaky0.9": (0.9, 0.013, 0.017, 0.011),
    "leaky0.1_shared": (0.1, 0.03, 0.041, 0.041),
}


def relu_pool_graph(seed, dims, k, s, p, caffe, slope, s_in, s_relu, s_pool, alg=0, glob=0, second_consumer=False, geom=None):
    """data -> ReLU(slope) -> Pooling; `second_consumer`: the ReLU's output is a graph output as well; `geom`: per-axis geometry of the
    pool (helpers.pool_geom) over k / s / p"""
    from helpers import pool_geom, pool_geom_out, pool_geom_params
    rng = np.random.default_rng(seed)
    G = pool_geom(geom, k, s, p)
    n, c, h, w = dims
    g = Graph(name="i8_relu_pool_case")
    x = g.add_input("data", list(dims), DT_INT8, [float(np.float32(s_in))], [0])
    r = g.add_tensor("act", list(dims), DT_INT8, tm2.TT_VAR, None, [float(np.float32(s_relu))], [0])
    ri = g.add_node("act", "ReLU", [x], [r], negative_slope=float(slope))
    if glob:
        G.update(kh=h, kw=w)
    oh, ow = pool_geom_out(h, w, G, glob, caffe)
    y = g.add_tensor("pooled", [n, c, oh, ow], DT_INT8, tm2.TT_VAR, None, [float(np.float32(s_pool))], [0])
    pi = g.add_node("pool", "Pooling", [r], [y], alg=alg, **{"global": glob}, caffe_flavor=caffe, **pool_geom_params(G))
    g.output_nodes = [pi, ri] if second_consumer else [pi]
    xin = rng.integers(-128, 128, size=dims).astype(np.int8)
    xin.flat[:min(256, xin.size)] = rng.permutation(np.arange(-128, 128))[:min(256, xin.size)]
    return g, xin


def relu_pool_concat_graph(seed, n=2, h=6, w=8):
    """data [n, 16, h, w] -> ReLU 0.1 -> max-pool 2x2 / 2 (carries the concat's scale: its output is a view at offset 32) --\\
                          -> conv(16 -> 32, 1x1, stride 2), the concat's scale                                            --> Concat"""
    rng = np.random.default_rng(seed)
    g = Graph(name="i8_relu_pool_concat_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    x = g.add_input("data", [n, 16, h, w], DT_INT8, [xs], [0])
    cat_s = float(np.float32(xs * 0.9))
    r = g.add_tensor("act", [n, 16, h, w], DT_INT8, tm2.TT_VAR, None, [float(np.float32(xs * 0.7))], [0])
    g.add_node("act", "ReLU", [x], [r], negative_slope=0.1)
    p = g.add_tensor("pooled", [n, 16, h // 2, w // 2], DT_INT8, tm2.TT_VAR, None, [cat_s], [0])
    g.add_node("pool", "Pooling", [r], [p], alg=0, kernel_h=2, kernel_w=2, stride_h=2, stride_w=2, **{"global": 0}, caffe_flavor=0,
               pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
    c = _conv(g, rng, "conv_side", x, 16, 32, h // 2, w // 2, n, stride=2, out_scale=cat_s)
    y = g.add_tensor("cat", [n, 48, h // 2, w // 2], DT_INT8, tm2.TT_VAR, None, [cat_s], [0])
    g.output_nodes = [g.add_node("route", "Concat", [c, p], [y], axis=1)]
    return g, rng.integers(-127, 128, size=(n, 16, h, w)).astype(np.int8)
