"""Seeded identity-bottleneck graphs for the block_i8 tests: a leading 1x1 conv (so that the block's input -- the residual -- is an
NHWC device tensor, not the raw graph input), then

    x - conv 1x1 (c -> mid) - conv 3x3 pad 1 (mid -> mid) - conv 1x1 (mid -> c) - Eltwise SUM with x - [ReLU]

and the variations the fusion must refuse."""
import numpy as np

from helpers import _scales, conv_geom, geom_params
from tengine_amd import tm2
from tengine_amd.tm2 import DT_INT8, DT_INT32, Graph


def _conv(g, rng, name, x, cin, cout, k, out_dims, act, bias, s=1, pad=0, dil=1, bias_range=(-2000, 2000), geom=None):
    """one group-1 convolution node behind tensor x; returns its output tensor.  Output scale as helpers.conv_graph sizes it.
    `geom`: per-axis overrides of the k x k / s / pad / dil geometry (helpers.conv_geom; the kernel stays k x k)"""
    G = conv_geom(geom, k, s, pad, dil)
    assert (G["kh"], G["kw"]) == (k, k)
    wq = rng.integers(-127, 128, size=(cout, cin, k, k)).astype(np.int8)
    ws = _scales(rng, cout)
    ins = [x, g.add_const(name + "_w", wq, DT_INT8, ws, [0] * cout)]
    if bias:
        ins.append(g.add_const(name + "_b", rng.integers(bias_range[0], bias_range[1], size=(cout,)).astype(np.int32), DT_INT32, [1.0], [0]))
    xs = g.tensors[x].scales[0]
    os_ = float(np.float32(xs * np.mean(ws) * 73.0 * np.sqrt(cin * k * k) * 73.0 / 60.0))
    y = g.add_tensor(name, out_dims, DT_INT8, tm2.TT_VAR, None, [os_], [0])
    g.add_node(name, "Convolution", ins, [y], input_channel=cin, output_channel=cout, group=1, activation=act, **geom_params(G))
    return y


def block_graph(seed, n, c, h, w, mid, act_lead=0, act_a=0, act_b=0, bias=True, relu=True, conv_first=False, relu_scale=1.0,
                stride_a=1, dil_b=1, projection=False, a_twice=False, b_is_output=False, bias_a_range=(-2000, 2000), cin0=16, geom_b=None):
    """returns (graph, input).  Tensor names: "x" the block input, "mid1" / "mid2" the two intermediate maps, "sum" the eltwise output,
    "out" the ReLU's.  conv_first: the Eltwise reads (branch2c, x) instead of (x, branch2c); relu_scale != 1: the ReLU re-quantises;
    stride_a 2 (with a stride-2 projection as the residual), dil_b 2, projection, a_twice (mid1 also feeds a ReLU that is a graph
    output), b_is_output (mid2 is a graph output): the shapes the fusion refuses.  geom_b: per-axis geometry of the 3x3 (it must
    keep the map size)."""
    rng = np.random.default_rng(seed)
    g = Graph(name="block_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    data = g.add_input("data", [n, cin0, h, w], DT_INT8, [xs], [0])
    x = _conv(g, rng, "x", data, cin0, c, 1, [n, c, h, w], act_lead, bias)
    oh, ow = (h - 1) // stride_a + 1, (w - 1) // stride_a + 1
    m1 = _conv(g, rng, "mid1", x, c, mid, 1, [n, mid, oh, ow], act_a, bias, s=stride_a, bias_range=bias_a_range)
    m2 = _conv(g, rng, "mid2", m1, mid, mid, 3, [n, mid, oh, ow], act_b, bias, pad=dil_b, dil=dil_b, geom=geom_b)
    y = _conv(g, rng, "branch2c", m2, mid, c, 1, [n, c, oh, ow], -1, bias)
    outs = []
    res = x
    if projection or stride_a != 1:
        res = _conv(g, rng, "branch1", x, c, c, 1, [n, c, oh, ow], -1, bias, s=stride_a)
    so = float(np.float32(max(g.tensors[res].scales[0], g.tensors[y].scales[0]) * 1.5))
    e = g.add_tensor("sum", [n, c, oh, ow], DT_INT8, tm2.TT_VAR, None, [so], [0])
    ni = g.add_node("sum", "Eltwise", [y, res] if conv_first else [res, y], [e], type=tm2.ELT_SUM, caffe_flavor=1)
    if relu:
        r = g.add_tensor("out", [n, c, oh, ow], DT_INT8, tm2.TT_VAR, None, [float(np.float32(so * relu_scale))], [0])
        ni = g.add_node("out", "ReLU", [e], [r], negative_slope=0.0)
    if a_twice:
        side = g.add_tensor("side", [n, mid, oh, ow], DT_INT8, tm2.TT_VAR, None, [g.tensors[m1].scales[0]], [0])
        outs.append(g.add_node("side", "ReLU", [m1], [side], negative_slope=0.0))
    if b_is_output:
        outs.append([i for i, nd in enumerate(g.nodes) if nd.outputs and nd.outputs[0] == m2][0])
    g.output_nodes = [ni] + outs
    xin = rng.integers(-127, 128, size=(n, cin0, h, w)).astype(np.int8)
    return g, xin


def tensor_index(g, name):
    return [i for i, t in enumerate(g.tensors) if t.name == name][0]


def requantised_bias(g, conv_name):
    """what a relu convolution stores where all its inputs are zero: relu(round(bias * in_scale * w_scale[c] / out_scale)) per channel,
    from the node's quantisation parameters (the value a kernel that padded branch2a's map with requant(bias) would put there)"""
    node = [nd for nd in g.nodes if nd.name == conv_name][0]
    xs = np.float32(g.tensors[node.inputs[0]].scales[0])
    ws = np.asarray(g.tensors[node.inputs[1]].scales, np.float32)
    b = np.asarray(g.tensors[node.inputs[2]].data).astype(np.float32).ravel()
    os_ = np.float32(g.tensors[node.outputs[0]].scales[0])
    f = np.maximum(b * xs * ws, np.float32(0))
    return np.clip(np.floor(f / os_ + np.float32(0.5)), -127, 127).astype(np.int32)
