"""Builders for the tests of the Eltwise forms that run by table -- a tensor against a constant one-element operand, and the unary
types -- (tests/test_bytemap_cpu.py, tests/test_gpu_bytemap.py, tools/make_golden_bytemap.py): single-node graphs with chosen
quantisation parameters and constants, the parameter sets of every (type, data type) pair, and small chains of convolutions with
these nodes between them.  Every case is tmfile bytes: the reference library and the device read the same model."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
import se_helpers as sh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bytemap_cases.npz")
f32 = lh.f32
TAG = {DT_INT8: "i8", DT_UINT8: "u8"}

SCALAR_TYPES = {"prod": 0, "prod_scalar": 1, "sum": 2, "sub": 4, "sub_scalar": 5, "min_scalar": 8, "div": 10}
UNARY_TYPES = {"rsqrt": 7, "log": 11, "exp": 12, "sqrt": 13, "floor": 14, "square": 15, "power": 17}
NAME = {v: k for k, v in list(SCALAR_TYPES.items()) + list(UNARY_TYPES.items())}


def all_bytes(dtype):
    """(1, 4, 8, 8): element i holds byte value i"""
    return np.arange(256, dtype=np.uint8).view(lh.NP[dtype]).reshape(1, 4, 8, 8)


def const_of(g, name, spec):
    """spec: ("u8", byte, scale, zp) | ("i8", q, scale) | ("f32", value); dims: spec[-1] where it is a list, else [1]"""
    dims = [1]
    if isinstance(spec[-1], list):
        spec, dims = spec[:-1], spec[-1]
    kind = spec[0]
    if kind == "u8":
        return g.add_const(name, np.full(dims, spec[1], np.uint8), DT_UINT8, [f32(spec[2])], [int(spec[3])])
    if kind == "i8":
        return g.add_const(name, np.full(dims, spec[1], np.int8), DT_INT8, [f32(spec[2])], [0])
    return g.add_const(name, np.full(dims, spec[1], np.float32), DT_FP32)


def const_value(spec):
    """the float the reference's kernels make of the constant (tamd_eltwise_scalar)"""
    if isinstance(spec[-1], list):
        spec = spec[:-1]
    if spec[0] == "u8":
        return capi.eltwise_scalar(DT_UINT8, np.uint8(spec[1]), f32(spec[2]), int(spec[3]))
    if spec[0] == "i8":
        return capi.eltwise_scalar(DT_INT8, np.int8(spec[1]), f32(spec[2]), 0)
    return capi.eltwise_scalar(DT_FP32, np.float32(spec[1]))


def node_graph(dtype, typ, dims, in_q, out_q, const=None, params=None, const_first=False, const_is_input=False):
    """input(dims) [, constant] -> Eltwise(typ) -> output.  const None: the unary form, one input"""
    g = Graph(name="bytemap_%s_case" % NAME.get(typ, "t%d" % typ))
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    ins = [x]
    if const is not None:
        if const_is_input:
            c = g.add_input("scalar", [1], dtype, *q((const[2], const[3] if len(const) > 3 else 0)))
        else:
            c = const_of(g, "scalar", const)
        ins = [c, x] if const_first else [x, c]
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, *q(out_q))
    g.output_nodes = [g.add_node("elt_" + NAME.get(typ, "t%d" % typ), "Eltwise", ins, [y], type=typ, caffe_flavor=1, **(params or {}))]
    return g


def table_of(typ, dtype, in_q, out_q, const=None, params=None):
    """(rc, bytes) of tamd_eltwise_table for the node node_graph builds"""
    p = params or {}
    s = const_value(const) if const is not None else 0.0
    return capi.eltwise_table(typ, dtype, s, f32(in_q[0]), int(in_q[1]), f32(out_q[0]), int(out_q[1]), f32(p.get("shift", 0.0)), f32(p.get("power", 1.0)),
                              f32(p.get("scale", 1.0)))


# ---- parameter sets: (id, type, dtype, in (scale, zp), out (scale, zp), constant spec | None, params | None) ----
# Every set's table is DEFINED in the reference: no NaN, no infinity, nothing outside int before the conversion.  That limits the
# unary types: SQRT needs x >= 0 on all 256 bytes and RSQRT / LOG x > 0 -- a uint8 tensor with zero point <= 0 (< 0), and NO int8
# tensor, whose bytes -128 .. 127 always reach negative values: int8 RSQRT / LOG / SQRT (and POWER with a fractional power) have no
# defined table on any parameters and are refused by that rule (UNDEFINED_INT8 below); EXP stays below exp(88).
def _scalar_sets():
    sets = []
    u8_io = [((0.05, 0), (0.05, 128)), ((0.05, 128), (0.01, 128)), ((0.03, 255), (0.02, 200)), ((0.1, 77), (0.2, 100)),
             ((0.02, 128), (0.004, 0)), ((0.02, 128), (0.004, 255)), ((0.07, 13), (0.11, 31)), ((0.013, 200), (0.009, 90))]
    u8_c = [("u8", 140, 0.05, 128), ("f32", 0.5), ("u8", 3, 0.01, 128), ("f32", -1.75), ("f32", 127.5 * 0.02), ("u8", 255, 0.0078125, 0), ("f32", 0.0078125), ("u8", 0, 0.02, 77)]
    i8_io = [((0.05, 0), (0.05, 0)), ((0.05, 0), (0.01, 0)), ((0.03, 0), (0.02, 0)), ((0.1, 0), (0.2, 0)),
             ((0.02, 0), (0.004, 0)), ((0.02, 0), (0.5, 0)), ((0.07, 0), (0.11, 0)), ((0.013, 0), (0.009, 0))]
    i8_c = [("i8", 12, 0.05), ("i8", -128, 0.01), ("i8", 3, 0.01), ("i8", -35, 0.05), ("i8", 127, 0.02), ("i8", 1, 0.0078125), ("i8", -1, 0.3), ("i8", 64, 0.02)]
    for name, typ in SCALAR_TYPES.items():
        for k in range(8):
            (iq, oq), c = u8_io[k], u8_c[(k + typ) % 8]
            sets.append(("%s_u8_%d" % (name, k), typ, DT_UINT8, iq, oq, c, None))
            (iq, oq), c = i8_io[k], i8_c[(k + typ) % 8]
            sets.append(("%s_i8_%d" % (name, k), typ, DT_INT8, iq, oq, c, None))
    return sets


def _unary_sets():
    sets = []
    pos = [(0.05, -1), (0.02, -3), (0.1, -1), (0.004, -10), (0.3, -1), (0.011, -2), (0.05, -200), (1.0, -1)]      # x > 0 on every byte
    nonneg = [(0.05, 0), (0.02, 0), (0.1, -5), (0.004, 0), (0.3, 0), (0.011, -2), (0.05, -200), (1.0, 0)]          # x >= 0
    anyq = [(0.05, 0), (0.05, 128), (0.03, 255), (0.1, 77), (0.02, 128), (0.3, 100), (0.07, 13), (0.013, 200)]
    outs = [(0.05, 0), (0.01, 0), (0.02, 200), (0.2, 100), (0.004, 0), (0.004, 255), (0.11, 31), (0.5, 3)]
    for k in range(8):
        o = outs[k]
        sets.append(("rsqrt_u8_%d" % k, 7, DT_UINT8, pos[k], o, None, None))
        sets.append(("log_u8_%d" % k, 11, DT_UINT8, pos[k], (o[0], 128 if k % 2 else o[1]), None, None))
        sets.append(("exp_u8_%d" % k, 12, DT_UINT8, (min(anyq[k][0], 0.05), anyq[k][1]), o, None, None))      # (x <= 12.75: e^x / 0.004 is inside int)
        sets.append(("sqrt_u8_%d" % k, 13, DT_UINT8, nonneg[k], o, None, None))
        sets.append(("floor_u8_%d" % k, 14, DT_UINT8, anyq[k], (1.0 if k % 2 else o[0], 128 if k < 4 else o[1]), None, None))
        sets.append(("square_u8_%d" % k, 15, DT_UINT8, anyq[k], o, None, None))
        pws = [{"shift": 0.0, "scale": 1.0, "power": 2.0}, {"shift": 1.5, "scale": 0.5, "power": 3.0}, {"shift": 8.0, "scale": 1.0, "power": 0.5},
               {"shift": 0.25, "scale": -2.0, "power": 2.0}, {"shift": 3.0, "scale": 1.0, "power": -1.0}, {"shift": 0.0, "scale": 1.0, "power": 1.0},
               {"shift": 1.0, "scale": 0.0625, "power": 5.0}, {"shift": 3.0, "scale": 0.3333, "power": 0.0}]
        # (base > 0 wherever the power is fractional or negative: set 2: x >= -6.4 + 8; set 4: (0.02, 128): x >= -2.56 + 3)
        pin = [anyq[0], anyq[1], (0.05, 128), anyq[3], (0.02, 128), anyq[5], anyq[6], anyq[7]][k]
        sets.append(("power_u8_%d" % k, 17, DT_UINT8, pin, o, None, pws[k]))
        io8 = [(0.05, 0.05), (0.05, 0.01), (0.03, 0.02), (0.1, 0.2), (0.02, 0.004), (0.3, 0.5), (0.07, 0.11), (0.013, 0.009)][k]
        sets.append(("exp_i8_%d" % k, 12, DT_INT8, (min(io8[0], 0.1), 0), (io8[1], 0), None, None))
        sets.append(("floor_i8_%d" % k, 14, DT_INT8, (io8[0], 0), (1.0 if k % 2 else io8[1], 0), None, None))
        sets.append(("square_i8_%d" % k, 15, DT_INT8, (io8[0], 0), (io8[1], 0), None, None))
        ipw = dict(pws[k], shift=9.0) if k == 4 else pws[k]
        iin = [0.05, 0.05, 0.05, 0.1, 0.05, 0.3, 0.07, 0.013][k]       # (sets 2 and 4: x >= -6.4: base > 0)
        sets.append(("power_i8_%d" % k, 17, DT_INT8, (iin, 0), (io8[1], 0), None, ipw))
    return sets


PARAM_SETS = _scalar_sets() + _unary_sets()
# the (type, int8) pairs whose table is undefined on every int8 tensor (the bytes reach negative values: NaN), with parameters to ask with
UNDEFINED_INT8 = [(7, (0.05, 0), (0.05, 0)), (11, (0.05, 0), (0.05, 0)), (13, (0.05, 0), (0.05, 0))]
RUNNING_PAIRS = sorted({(s[1], s[2]) for s in PARAM_SETS})


class Chain(lh.Chain):
    """lut_helpers.Chain with the scalar and unary Eltwise nodes"""

    def _const(self, value, kind=None):
        """a one-element constant near `value`: uint8 graphs take an fp32 one (kind "f32") or a uint8 one, int8 graphs an int8 one"""
        self.k += 1
        name = "c%d" % self.k
        if self.dtype == DT_UINT8 and kind == "f32":
            return const_of(self.g, name, ("f32", value)), f32(value)
        if self.dtype == DT_UINT8:
            scale = f32(abs(value) / 100.0) if value else f32(0.01)
            spec = ("u8", 128 + int(round(value / scale)), scale, 128)
        else:
            scale = f32(abs(value) / 100.0) if value else f32(0.01)
            spec = ("i8", int(round(value / scale)), scale)
        return const_of(self.g, name, spec), const_value(spec)

    def scalar(self, typ, value, out_q, kind=None, src=None):
        x = self.cur if src is None else src
        c, _ = self._const(value, kind)
        name = self._name(NAME[typ])
        y = self._var(name, self.dims(x), out_q)
        self.last = self.g.add_node(name, "Eltwise", [x, c], [y], type=typ, caffe_flavor=1)
        self.cur = y
        return y

    def unary(self, typ, out_q, **params):
        name = self._name(NAME[typ])
        y = self._var(name, self.dims(), out_q)
        self.last = self.g.add_node(name, "Eltwise", [self.cur], [y], type=typ, caffe_flavor=1, **params)
        self.cur = y
        return y

    def binary(self, typ, a, b, out_q):
        name = self._name("elt")
        y = self._var(name, self.dims(a), out_q)
        self.last = self.g.add_node(name, "Eltwise", [a, b], [y], type=typ, caffe_flavor=1)
        self.cur = y
        return y


def zp(dtype, v):
    return 0 if dtype == DT_INT8 else v


def normalise_graph(dtype, dims=(2, 3, 6, 6)):
    """MobileFaceNet's front: input -> SUB_SCALAR 127.5 -> PROD_SCALAR 0.0078125 -> conv 3x3 -> conv 1x1 (uint8: fp32 constants, as the
    file has them; int8: int8 constants on an input of scale 1)"""
    c = Chain(41, dtype, dims, in_q=(1.0, 0))
    if dtype == DT_UINT8:
        c.scalar(5, 127.5, (1.0, 128), kind="f32")
        c.scalar(1, 0.0078125, (0.0078125, 128), kind="f32")
    else:
        c.scalar(5, 20.0, (1.2, 0))
        c.scalar(1, 0.0078125, (0.0078125 * 1.2, 0))
    c.conv(8, 3, 1); c.conv(6, 1)
    return c.done()


def hardswish_graph(dtype, dims=(1, 16, 7, 7), div=False):
    """conv -> [SUM 3 -> Clip(0, 6) -> PROD(x, .) -> PROD_SCALAR 1/6 (uint8 with div: -> DIV 6 instead)] -> conv: the decomposed HardSwish of
    a torch export"""
    c = Chain(42, dtype, dims)
    x = c.conv(dims[1], 3, 1)
    s = c.scale(x)
    c.scalar(2, 3.0, (s * 1.1, zp(dtype, 100)))
    t = c.act("Clip")
    c.binary(tm2.ELT_PROD, x, t, (s * 3.0, zp(dtype, 60)))
    if div:
        c.scalar(10, 6.0, (s * 0.6, zp(dtype, 60)), kind="f32")
    else:
        c.scalar(1, 1.0 / 6.0, (s * 0.6, zp(dtype, 60)))
    c.conv(8, 1)
    return c.done()


def unary_chain_graph(dtype, dims=(1, 8, 6, 6)):
    """conv -> SQUARE -> FLOOR -> conv: the unary form between convolutions"""
    c = Chain(43, dtype, dims)
    x = c.conv(8, 3, 1)
    s = c.scale(x)
    c.unary(15, (s * s * 60.0, zp(dtype, 5)))
    c.unary(14, (s * s * 120.0, zp(dtype, 9)))
    c.conv(6, 1)
    return c.done()


def silu_graph(dtype, dims=(2, 8, 5, 3), sigmoid_is_output=False, mid=16):
    """conv -> Sigmoid -> Eltwise PROD(conv, sigmoid) -> conv: SiLU, the activation of YOLOv5 / YOLOX, between two convolutions.
    sigmoid_is_output: the Sigmoid's tensor is a graph output too (it must be written: no chain)"""
    c = Chain(45, dtype, dims)
    a = c.conv(mid, 3, 1)
    s = c.act("Sigmoid")
    sig_node = c.last
    c.prod(a, s)
    c.conv(8, 1)
    g, x = c.done()
    if sigmoid_is_output:
        g.output_nodes = [c.last, sig_node]
    return g, x


def hardswish_second_reader_graph(dtype, dims=(1, 16, 7, 7)):
    """the HardSwish decomposition whose Clip output has a second reader (a convolution, the second graph output): the chain ends at the
    Clip -- SUM 3 -> Clip as one launch, then PROD and PROD_SCALAR by themselves"""
    c = Chain(46, dtype, dims)
    x = c.conv(dims[1], 3, 1)
    s = c.scale(x)
    c.scalar(2, 3.0, (s * 1.1, zp(dtype, 100)))
    t = c.act("Clip")
    c.conv(4, 1, src=t)
    side = c.last
    c.binary(tm2.ELT_PROD, x, t, (s * 3.0, zp(dtype, 60)))
    c.scalar(1, 1.0 / 6.0, (s * 0.6, zp(dtype, 60)))
    c.conv(8, 1)
    g, xin = c.done()
    g.output_nodes = [c.last, side]
    return g, xin


def two_branch_graph(dtype, dims=(1, 8, 6, 5), side_reader=False):
    """conv -> [Clip(0, 6) of it, Sigmoid of it] -> PROD(clip, sigmoid) -> conv: two table nodes that both read the source, then a
    same-shape node over them -- one chain of three.  side_reader: the Sigmoid is ALSO a graph output and the product is replaced by a
    SQUARE behind the Clip: the chain is Clip -> SQUARE, and the Sigmoid between them in node order stays a launch of its own"""
    c = Chain(47, dtype, dims)
    x = c.conv(dims[1], 3, 1)
    a = c.act("Clip")
    c.cur = x
    b = c.act("Sigmoid")
    sig_node = c.last
    if side_reader:
        c.cur = a
        c.unary(15, (0.15, zp(dtype, 3)))                      # (clip(x)^2 in [0, 36]: 240 steps of 0.15)
    else:
        c.binary(tm2.ELT_PROD, a, b, (c.scale(a) * 0.6, zp(dtype, 4)))
    c.conv(6, 1)
    g, xin = c.done()
    if side_reader:
        g.output_nodes = [c.last, sig_node]
    return g, xin


def chain_start(g):
    """the index of the first table node (Sigmoid / Clip / scalar or unary Eltwise) of the graph"""
    for i, n in enumerate(g.nodes):
        if n.op in ("Sigmoid", "Clip", "HardSwish", "Mish") or (n.op == "Eltwise" and (len(n.inputs) == 1 or g.tensors[n.inputs[1]].ttype == tm2.TT_CONST)):
            return i
    raise ValueError("no table node")


def node_table(g, n):
    """the byte map of one table node between its two tensors, from the single-node builders (tamd_lut_table / tamd_eltwise_table)"""
    x, y = g.tensors[n.inputs[0]], g.tensors[n.outputs[0]]
    iq, oq = (x.scales[0], x.zero_points[0]), (y.scales[0], y.zero_points[0])
    if n.op != "Eltwise":
        return lh.table_of(capi, n.op, x.dtype, iq, oq, {k: v for k, v in n.params.items()})
    s = 0.0
    if len(n.inputs) == 2:
        c = g.tensors[n.inputs[1]]
        s = capi.eltwise_scalar(c.dtype, c.data, c.scales[0] if c.scales else 0.0, c.zero_points[0] if c.zero_points else 0)
    rc, tab = capi.eltwise_table(n.params["type"], x.dtype, s, iq[0], iq[1], oq[0], oq[1], n.params.get("shift", 0.0), n.params.get("power", 1.0), n.params.get("scale", 1.0))
    assert rc == 0
    return tab


def compose(g, members):
    """the chain's table composed node by node in Python: table2[table1[b]] for table nodes, tamd_eltwise_pair on the two operands'
    bytes for the same-shape nodes.  members: node indices in order; the source is the first member's input"""
    src = g.nodes[members[0]].inputs[0]
    val = {src: np.arange(256, dtype=np.uint8)}
    for ni in members:
        n = g.nodes[ni]
        y = n.outputs[0]
        if n.op == "Eltwise" and len(n.inputs) == 2 and g.tensors[n.inputs[1]].ttype != tm2.TT_CONST:
            a, b, o = (g.tensors[i] for i in (n.inputs[0], n.inputs[1], y))
            q = lambda t: (t.scales[0], t.zero_points[0])
            val[y] = np.array([capi.eltwise_pair(n.params["type"], a.dtype, va, q(a), vb, q(b), q(o)) for va, vb in zip(val[n.inputs[0]], val[n.inputs[1]])], dtype=np.uint8)
        else:
            val[y] = node_table(g, n)[val[n.inputs[0]]]
    return val[g.nodes[members[-1]].outputs[0]]


def geometry_case(dtype, typ, dims, seed, const=None, in_q=None, out_q=None, params=None):
    in_q = in_q or ((0.05, 0) if dtype == DT_INT8 else (0.05, 128))
    out_q = out_q or ((0.04, 0) if dtype == DT_INT8 else (0.04, 120))
    return node_graph(dtype, typ, dims, in_q, out_q, const, params), [lh.random_bytes(seed, dtype, dims)]


def padding_graph(dims=(2, 8, 5, 3)):
    """int8 conv1x1 (8 -> 5) -> SUM 0.7 -> conv3x3 pad 1 (5 -> 7): the 5-channel tensors have 11 padding lanes per pixel on the device, the
    table maps byte 0 to a non-zero byte, and the second convolution's K loop reads the lanes lut_u8 must have written as zero"""
    c = Chain(44, DT_INT8, dims)
    x = c.conv(5, 1)
    c.scalar(2, 0.7, (c.scale(x) * 1.3, 0))
    c.conv(7, 3, 1)
    return c.done()


def _one(gx):
    g, x = gx
    return g, [x]


def _set_case(s, dims=None):
    _, typ, dtype, iq, oq, const, params = s
    if dims is None:
        return node_graph(dtype, typ, (1, 4, 8, 8), iq, oq, const, params), [all_bytes(dtype)]
    return node_graph(dtype, typ, dims, iq, oq, const, params), [lh.random_bytes(typ + 7, dtype, dims)]


def gpu_cases():
    """{id: (dtype, builder)}: every graph the GPU tests run against the reference; a builder returns (graph, [inputs]).  Each running
    (type, data type) pair alone on the tensor that holds all 256 bytes and on (2, 5, 3, 3) -- 90 bytes, a ragged last vector; int8: 11
    padding lanes per pixel --, with the pair's parameter set number 1 (the scalar ones saturate at both ends there)"""
    cases = {}
    first = {}
    for s in PARAM_SETS:
        if s[0].endswith("_1"):
            first[(s[1], s[2])] = s
    for (typ, dtype), s in sorted(first.items()):
        cases["all_%s_%s" % (TAG[dtype], NAME[typ])] = (dtype, lambda s=s: _set_case(s))
        cases["ragged_%s_%s" % (TAG[dtype], NAME[typ])] = (dtype, lambda s=s: _set_case(s, (2, 5, 3, 3)))
    for dt in (DT_INT8, DT_UINT8):
        cases["%s_normalise" % TAG[dt]] = (dt, lambda dt=dt: _one(normalise_graph(dt)))
        cases["%s_hardswish" % TAG[dt]] = (dt, lambda dt=dt: _one(hardswish_graph(dt)))
        cases["%s_unary_chain" % TAG[dt]] = (dt, lambda dt=dt: _one(unary_chain_graph(dt)))
        cases["%s_silu" % TAG[dt]] = (dt, lambda dt=dt: _one(silu_graph(dt)))
        cases["%s_silu_sigmoid_is_output" % TAG[dt]] = (dt, lambda dt=dt: _one(silu_graph(dt, sigmoid_is_output=True)))
        cases["%s_hardswish_second_reader" % TAG[dt]] = (dt, lambda dt=dt: _one(hardswish_second_reader_graph(dt)))
        cases["%s_two_branches" % TAG[dt]] = (dt, lambda dt=dt: _one(two_branch_graph(dt)))
        cases["%s_branch_beside_a_chain" % TAG[dt]] = (dt, lambda dt=dt: _one(two_branch_graph(dt, side_reader=True)))
    cases["u8_hardswish_div"] = (DT_UINT8, lambda: _one(hardswish_graph(DT_UINT8, div=True)))
    cases["i8_padding"] = (DT_INT8, lambda: _one(padding_graph()))
    for k, d in enumerate(BN_SHAPES):                      # the BatchNorm between its guards, and MobileFaceNet's two ends at batch 1 and 2
        cases["bn_" + "x".join(map(str, d))] = (DT_UINT8, lambda d=d, k=k: _one(bn_guarded_graph(d, 30 + k)[:2]))
    for n in (1, 2):
        cases["u8_mobilefacenet_ends_b%d" % n] = (DT_UINT8, lambda n=n: _one(mobilefacenet_ends_graph(n)))
    return cases


reference_outputs = sh.reference_outputs
device_outputs = sh.device_outputs
golden_entry = sh.golden_entry
equals_golden = ih.equals_golden
library_error = sh.library_error
library_output_shape = sh.library_output_shape


def golden():
    return np.load(GOLDEN)


def child_main(case, path):
    """what a fresh child process runs for the GPU tests (python -c ...: the environment it was started with decides the plan): the case
    through the C ABI, its outputs and kernel names saved to `path`"""
    dtype, build = gpu_cases()[case]
    g, xs = build()
    out, names, _ = device_outputs(tm2.write_tm2(g), xs)
    np.savez(path, names=np.array(names), **{"out%d" % i: o for i, o in enumerate(out)})


def _desc(dtype, dims, ttype=1, quant=None, q=None, data=None, keep=None):
    d = sh._desc(dtype, dims, ttype, quant)
    if q is not None:
        sc, z = (C.c_float * 1)(f32(q[0])), (C.c_int * 1)(int(q[1]))
        keep += [sc, z]
        d.scales, d.zero_points = C.cast(sc, C.c_void_p), C.cast(z, C.c_void_p)
    if data is not None:
        buf = np.ascontiguousarray(data)
        keep.append(buf)
        d.data = buf.ctypes.data_as(C.c_void_p)
    return d


def ask_node(dtype, typ, x_dims, const=None, in_q=None, out_q=None, params=None, out_dims=None, x_quant=None, out_quant=None, const_first=False, const_var=False,
             with_param=True, x_const=False):
    """tamd_node_supported for an Eltwise node [x (, constant)]; const: a const_of spec (its payload and pair are handed over), in_q /
    out_q: where given, the values are handed over too and the table is checked"""
    keep = []
    p = sh.EltwiseParam(typ, 1, *(f32((params or {}).get(k, d)) for k, d in (("shift", 0.0), ("power", 1.0), ("scale", 1.0))))
    n = lh.NodeDesc()
    n.op, n.output_num = sh.OP_ELTWISE, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    descs = [_desc(dtype, x_dims, 2 if x_const else 1, x_quant, in_q, keep=keep)]
    if const is not None:
        cdims = [1]
        spec = const
        if isinstance(spec[-1], list):
            spec, cdims = spec[:-1], spec[-1]
        if spec[0] == "u8":
            cd = _desc(DT_UINT8, cdims, 1 if const_var else 2, 1, (spec[2], spec[3]), np.full(cdims, spec[1], np.uint8), keep)
        elif spec[0] == "i8":
            cd = _desc(DT_INT8, cdims, 1 if const_var else 2, 1, (spec[2], 0), np.full(cdims, spec[1], np.int8), keep)
        else:
            cd = _desc(DT_FP32, cdims, 1 if const_var else 2, 0, None, np.full(cdims, spec[1], np.float32), keep)
        descs = [cd, descs[0]] if const_first else [descs[0], cd]
    n.input_num = len(descs)
    ins = (lh.TensorDesc * len(descs))(*descs)
    out = (lh.TensorDesc * 1)(_desc(dtype, out_dims or x_dims, quant=out_quant, q=out_q, keep=keep))
    return capi.lib().tamd_node_supported(C.byref(n), ins, len(descs), out, 1)


# ---- uint8 BatchNorm (tm2 operator 1): a byte map per channel ----

def bn_stats(C, seed, tiny_var=True):
    """gamma and beta of mixed sign, means around 0, variances from tiny to large: (gamma, beta, mean, var), float32 [C]"""
    r = np.random.default_rng(seed)
    gamma = (r.uniform(0.2, 2.0, C) * r.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = r.uniform(-1.5, 1.5, C).astype(np.float32)
    mean = r.uniform(-1.0, 1.0, C).astype(np.float32)
    var = r.uniform(0.05, 4.0, C).astype(np.float32)
    if tiny_var:
        var[::5] = np.float32(1e-7)
    return gamma, beta, mean, var


def bn_graph(dims, in_q, out_q, stats, rescale_factor=1.0, eps=1e-5, caffe_flavor=0, dtype=DT_UINT8, stat_dtype=DT_FP32, stat_len=None, stat_var=False):
    """input(dims) -> BatchNormalization [x, gamma, beta, mean, var] -> output.  stat_dtype / stat_len / stat_var: what a refused node
    carries instead (statistics of another type or length, or var a graph input)"""
    g = Graph(name="bytemap_batchnorm_case")
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    ins = [x]
    for name, v in zip(("gamma", "beta", "mean", "var"), stats):
        v = np.asarray(v, np.float32)[:stat_len] if stat_len else np.asarray(v, np.float32)
        if stat_var and name == "var":
            ins.append(g.add_input(name, [len(v)], dtype, *q((0.05, 0))))
        elif stat_dtype == DT_FP32:
            ins.append(g.add_const(name, v, DT_FP32))
        else:
            ins.append(g.add_const(name, np.clip(v * 20, 0, 255), stat_dtype, [f32(0.05)], [0]))
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, *q(out_q))
    g.output_nodes = [g.add_node("fc1_bn", "BatchNormalization", ins, [y], rescale_factor=rescale_factor, eps=eps, caffe_flavor=caffe_flavor)]
    return g


def bn_tables(C, in_q, out_q, stats, rescale_factor=1.0, eps=1e-5, caffe_flavor=0):
    """[C][256]: tamd_batchnorm_table of every channel"""
    gamma, beta, mean, var = stats
    out = np.zeros((C, 256), np.uint8)
    for c in range(C):
        rc, t = capi.batchnorm_table(float(gamma[c]), float(beta[c]), float(mean[c]), float(var[c]), f32(in_q[0]), int(in_q[1]), f32(out_q[0]), int(out_q[1]),
                                     f32(rescale_factor), f32(eps), caffe_flavor)
        assert rc == 0, (c, rc)
        out[c] = t
    return out


def bn_all_bytes(rank, C=16):
    """a tensor of the rank whose every channel holds all 256 bytes: [256, C], [1, C, 256] or (1, C, 16, 16)"""
    if rank == 2:
        return np.repeat(np.arange(256, dtype=np.uint8)[:, None], C, axis=1).copy()
    b = np.tile(np.arange(256, dtype=np.uint8), C)
    return b.reshape(1, C, 256) if rank == 3 else b.reshape(1, C, 16, 16)


def bn_apply(tables, x):
    """y[n, c, ...] = tables[c][x[n, c, ...]]"""
    C = x.shape[1]
    idx = np.arange(C).reshape((1, C) + (1,) * (x.ndim - 2))
    return tables[np.broadcast_to(idx, x.shape), x]


# (id, in (scale, zp), out (scale, zp), rescale_factor, eps, caffe_flavor)
BN_SETS = [
    ("mx_fc1", (0.05, 128), (0.04, 128), 1.0, 2e-5, 0), ("rescale_0", (0.05, 128), (0.02, 100), 0.0, 1e-3, 0), ("caffe", (0.03, 77), (0.03, 120), 1.0, 1e-5, 1),
    ("caffe_rescale_0", (0.05, 128), (0.05, 128), 0.0, 0.25, 1), ("rescale_half", (0.02, 0), (0.05, 30), 0.5, 1e-5, 0), ("saturating", (0.1, 128), (0.01, 128), 1.0, 1e-5, 0),
]


def bn_guarded_graph(dims, seed, in_q=(0.05, 128), out_q=(0.04, 120), caffe_flavor=0):
    """the BatchNorm between two guard regions: Clip(x) -> a, BatchNorm(x) -> y, Clip(x) -> b, the three tensors made in that order (the
    uint8 planner allocates in tensor order, so a and b lie on either side of y) and the BatchNorm planned LAST, so that a byte it wrote
    outside y would destroy what the comparison sees of a or b.  Outputs [a, y, b]"""
    g = Graph(name="bytemap_batchnorm_guarded")
    q = lambda v: ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), DT_UINT8, *q(in_q))
    a = g.add_tensor("guard_a", list(dims), DT_UINT8, tm2.TT_VAR, None, *q((0.03, 10)))
    y = g.add_tensor("out", list(dims), DT_UINT8, tm2.TT_VAR, None, *q(out_q))
    b = g.add_tensor("guard_b", list(dims), DT_UINT8, tm2.TT_VAR, None, *q((0.02, 3)))
    na = g.add_node("guard_a", "Clip", [x], [a], max=6.0, min=0.0)
    nb = g.add_node("guard_b", "Clip", [x], [b], max=3.0, min=-3.0)
    st = bn_stats(dims[1], seed)
    ins = [x] + [g.add_const(name, v, DT_FP32) for name, v in zip(("gamma", "beta", "mean", "var"), st)]
    ny = g.add_node("bn", "BatchNormalization", ins, [y], rescale_factor=1.0, eps=2e-5, caffe_flavor=caffe_flavor)
    g.output_nodes = [na, ny, nb]
    return g, lh.random_bytes(seed, DT_UINT8, dims), (st, in_q, out_q)


BN_SHAPES = [(3, 130), (2, 5, 7), (2, 5, 3, 3), (1, 3, 1, 17), (1, 2, 8, 40)]


def _ends_class():
    import prelu_helpers as ph

    class Ends(Chain, ph.Face):
        """the scalar / unary Eltwise nodes, PReLU and the residual sum in one builder, plus a strided convolution and a uint8 FC"""

        def conv_s(self, cout, k, stride, pad, group=1):
            g, rng = self.g, self.rng
            x = self.cur
            n, cin, h, w = self.dims(x)
            name = self._name("conv")
            fan = (cin // group) * k * k
            xs = self.scale(x)
            ws, wz = f32(rng.uniform(0.002, 0.02)), int(rng.integers(112, 144))
            ins = [x, g.add_const(name + "_w", rng.integers(0, 256, size=(cout, cin // group, k, k)), DT_UINT8, [ws], [wz]),
                   g.add_const(name + "_b", rng.integers(-4000, 4000, size=(cout,)), tm2.DT_INT32, [f32(np.float32(xs) * np.float32(ws))], [0])]
            oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
            y = self._var(name, [n, cout, oh, ow], (xs * ws * 73.0 * np.sqrt(fan) * 73.0 / 40.0, int(rng.integers(100, 156))))
            self.last = g.add_node(name, "Convolution", ins, [y], kernel_h=k, kernel_w=k, stride_h=stride, stride_w=stride, dilation_h=1, dilation_w=1,
                                   input_channel=cin, output_channel=cout, group=group, activation=-1, pad_h0=pad, pad_w0=pad, pad_h1=pad, pad_w1=pad)
            self.cur = y
            return y

        def fc_u8(self, nout):
            g, rng = self.g, self.rng
            d = self.dims()
            hidden = int(np.prod(d[1:]))
            xs = self.scale()
            ws, wz = f32(rng.uniform(0.002, 0.02)), int(rng.integers(112, 144))
            ins = [self.cur, g.add_const("pre_fc1_w", rng.integers(0, 256, size=(nout, hidden)), DT_UINT8, [ws], [wz]),
                   g.add_const("pre_fc1_b", rng.integers(-4000, 4000, size=(nout,)), tm2.DT_INT32, [f32(np.float32(xs) * np.float32(ws))], [0])]
            y = self._var("pre_fc1", [d[0], nout], (xs * ws * 73.0 * np.sqrt(hidden) * 73.0 / 40.0, int(rng.integers(100, 156))))
            self.last = g.add_node("pre_fc1", "FullyConnected", ins, [y], num_output=nout)
            self.cur = y
            return y

        def batchnorm(self, out_q, seed=5, eps=2e-5):
            x = self.cur
            C = self.dims(x)[1]
            st = bn_stats(C, seed, tiny_var=False)
            ins = [x] + [self.g.add_const("fc1_" + name, v, DT_FP32) for name, v in zip(("gamma", "beta", "mean", "var"), st)]
            y = self._var("fc1", self.dims(x), out_q)
            self.last = self.g.add_node("fc1", "BatchNormalization", ins, [y], rescale_factor=1.0, eps=eps, caffe_flavor=0)
            self.cur = y
            return y

    return Ends


def mobilefacenet_ends_graph(n=1, size=14, dtype=DT_UINT8):
    """MobileFaceNet's two ends as one graph, with the file's own node parameters.  Front: input (N, 3, size, size) -> SUB_SCALAR 127.5 ->
    PROD_SCALAR 0.0078125 -> conv 3x3 s2 p1 (64) -> PReLU.  Body: a bottleneck (conv 1x1 -> PReLU -> depthwise 3x3 -> PReLU -> conv 1x1)
    with its Eltwise SUM.  Tail: conv 1x1 (128) -> PReLU -> depthwise 7x7 on the 7x7 map -> FullyConnected 128 -> BatchNorm (eps 2e-5,
    rescale 1, not caffe).  size 14 -> a 7x7 map behind the stride-2 convolution; 112 is the file's own size (then the depthwise runs on
    the 56x56 map's 7x7 windows: the map is pooled by a stride-8 depthwise 7x7 first -- only the profile uses that)"""
    c = _ends_class()(48, dtype, (n, 3, size, size), in_q=(1.0, 0))
    if dtype == DT_UINT8:
        c.scalar(5, 127.5, (1.0, 128), kind="f32")
        c.scalar(1, 0.0078125, (0.0078125, 128), kind="f32")
    else:
        c.scalar(5, 20.0, (1.2, 0))
        c.scalar(1, 0.0078125, (0.0078125 * 1.2, 0))
    if dtype != DT_UINT8:
        raise ValueError("the ends graph is built for uint8 (int8 has no BatchNorm kernel in the reference)")
    c.conv_s(64, 3, 2, 1); c.prelu()
    data = c.cur
    c.conv(128, 1); c.prelu(); c.conv(128, 3, 1, group=128); c.prelu()
    y = c.conv(64, 1)
    c.add(data, y)
    c.conv(128, 1); c.prelu()
    h = c.dims()[2]
    if h > 7:
        c.conv_s(128, 7, 8 if h >= 56 else 1, 0, group=128)
        h = c.dims()[2]
    c.conv_s(128, c.dims()[2], 1, 0, group=128)
    c.fc_u8(128)
    c.batchnorm((0.05, 128))
    return c.done()
