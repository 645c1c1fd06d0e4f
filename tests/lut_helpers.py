"""Builders for the tests of the quantised Sigmoid / Clip / HardSwish / Mish nodes (tests/test_lut_cpu.py, tests/test_gpu_lut.py):
single-node graphs with chosen quantisation parameters, the parameter sets that reach every branch of the reference kernels, and small
chains of convolutions with the four operators between them.  Every case is tmfile bytes: the reference library and the device read
the same model."""
import ctypes as C

import numpy as np

from tengine_amd import tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_INT32, DT_UINT8, Graph

OPCODE = {"Sigmoid": 16, "Clip": 17, "HardSwish": 18, "Mish": 19}          # TAMD_OP_*
NP = {DT_INT8: np.int8, DT_UINT8: np.uint8, DT_FP32: np.float32}
# the six (operator, type) pairs the reference has a quantised kernel for
PAIRS = [("Sigmoid", DT_INT8), ("Sigmoid", DT_UINT8), ("Clip", DT_INT8), ("Clip", DT_UINT8), ("HardSwish", DT_UINT8), ("Mish", DT_UINT8)]
DEFAULT_PARAMS = {"Sigmoid": {}, "Mish": {}, "Clip": {"max": 6.0, "min": 0.0}, "HardSwish": {"alpha": 1.0, "beta": 3.0}}


def f32(v):
    return float(np.float32(v))


def ref_mode(ref, dtype):
    return {DT_INT8: ref.MODE_INT8, DT_UINT8: ref.MODE_UINT8, DT_FP32: ref.MODE_FP32}[dtype]


def unary_graph(op, dtype, dims, in_q, out_q, params=None):
    """input(dims) -> op -> output; in_q / out_q: (scale, zero point)"""
    g = Graph(name="lut_%s_case" % op.lower())
    x = g.add_input("data", list(dims), dtype, [f32(in_q[0])], [int(in_q[1])])
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, [f32(out_q[0])], [int(out_q[1])])
    g.output_nodes = [g.add_node(op.lower(), op, [x], [y], **(DEFAULT_PARAMS[op] if params is None else params))]
    return g


def all_bytes(dtype):
    """(1, 16, 4, 4): element i holds byte value i"""
    return np.arange(256, dtype=np.uint8).view(NP[dtype]).reshape(1, 16, 4, 4)


def random_bytes(seed, dtype, dims):
    """every byte value, -128 included: the reference kernels take whatever the tensor holds"""
    return np.random.default_rng(seed).integers(0, 256, size=dims).astype(np.uint8).view(NP[dtype])


# (id, operator, type, (in scale, in zp), (out scale, out zp), params).  What each set is for is in its id; the arithmetic behind the
# Clip sets: Clip(0, 6) at out scale 0.03 gives quotients up to 200 (128 .. 255 wrap negative in int8), at 0.02 up to 300 (> 255
# saturates to 255 == -1); in uint8 an input zero point of 200 with Clip(-3, 3) and out zp 0 makes the clipped value quantise below 0
PARAM_SETS = [
    ("sigmoid_i8_a", "Sigmoid", DT_INT8, (0.05, 0), (1 / 127.0, 0), None),
    ("sigmoid_i8_b", "Sigmoid", DT_INT8, (0.11, 0), (0.004, 0), None),
    ("sigmoid_i8_beyond_30", "Sigmoid", DT_INT8, (0.3, 0), (1 / 127.0, 0), None),           # |x| up to 38: the clamp lines
    ("sigmoid_u8_zp0", "Sigmoid", DT_UINT8, (0.05, 0), (1 / 256.0, 0), None),
    ("sigmoid_u8_zp128", "Sigmoid", DT_UINT8, (0.05, 128), (1 / 256.0, 0), None),
    ("sigmoid_u8_zp255", "Sigmoid", DT_UINT8, (0.05, 255), (1 / 256.0, 0), None),
    ("clip6_i8_fits", "Clip", DT_INT8, (0.06, 0), (6 / 127.0, 0), {"max": 6.0, "min": 0.0}),
    ("clip6_i8_wraps_negative", "Clip", DT_INT8, (0.06, 0), (0.03, 0), {"max": 6.0, "min": 0.0}),
    ("clip6_i8_above_255", "Clip", DT_INT8, (0.06, 0), (0.02, 0), {"max": 6.0, "min": 0.0}),
    ("clip_pm1_i8", "Clip", DT_INT8, (0.02, 0), (1 / 127.0, 0), {"max": 1.0, "min": -1.0}),
    ("clip6_u8_zp0", "Clip", DT_UINT8, (0.05, 30), (6 / 255.0, 0), {"max": 6.0, "min": 0.0}),
    ("clip6_u8_zp100", "Clip", DT_UINT8, (0.05, 30), (0.04, 100), {"max": 6.0, "min": 0.0}),
    ("clip_u8_below_0", "Clip", DT_UINT8, (0.05, 200), (0.05, 0), {"max": 3.0, "min": -3.0}),
    ("clip_pm1_u8", "Clip", DT_UINT8, (0.02, 128), (1 / 127.0, 128), {"max": 1.0, "min": -1.0}),
    ("hardswish_u8_zp0", "HardSwish", DT_UINT8, (0.04, 0), (0.05, 10), None),
    ("hardswish_u8_zp77", "HardSwish", DT_UINT8, (0.05, 77), (0.031, 12), None),
    ("hardswish_u8_zp255", "HardSwish", DT_UINT8, (0.03, 255), (0.004, 100), None),
    ("hardswish_u8_alpha_beta_ignored", "HardSwish", DT_UINT8, (0.05, 77), (0.031, 12), {"alpha": 0.25, "beta": 0.75}),
    ("mish_u8_zp0", "Mish", DT_UINT8, (0.04, 0), (0.05, 10), None),
    ("mish_u8_zp77", "Mish", DT_UINT8, (0.05, 77), (0.031, 12), None),
    ("mish_u8_zp255", "Mish", DT_UINT8, (0.03, 255), (0.004, 100), None),
]


def table_of(capi, op, dtype, in_q, out_q, params):
    p = DEFAULT_PARAMS[op] if params is None else params
    pair = (p["max"], p["min"]) if op == "Clip" else (p["alpha"], p["beta"]) if op == "HardSwish" else None
    return capi.lut_table(OPCODE[op], dtype, f32(in_q[0]), int(in_q[1]), f32(out_q[0]), int(out_q[1]), pair)


class Chain:
    """a graph grown node by node from one input; `dtype` decides the quantisation form of every tensor (fp32: none).  The output
    scale of a convolution spreads its results over the byte range without saturating everywhere (helpers.conv_graph's recipe)."""

    def __init__(self, seed, dtype, dims, in_q=None):
        self.rng = np.random.default_rng(seed)
        self.dtype, self.g, self.k = dtype, Graph(name="lut_chain"), 0
        q = in_q or ((f32(self.rng.uniform(0.01, 0.05)), 0) if dtype == DT_INT8 else (f32(self.rng.uniform(0.01, 0.05)), int(self.rng.integers(112, 144))))
        self.cur = self.g.add_input("data", list(dims), dtype, *self._q(q))
        self.last = None

    def _q(self, q):
        return (None, None) if self.dtype == DT_FP32 else ([f32(q[0])], [int(q[1])])

    def _name(self, base):
        self.k += 1
        return "%s%d" % (base, self.k)

    def dims(self, t=None):
        return list(self.g.tensors[self.cur if t is None else t].dims)

    def scale(self, t=None):
        return self.g.tensors[self.cur if t is None else t].scales[0]

    def _var(self, name, dims, q):
        return self.g.add_tensor(name, list(dims), self.dtype, tm2.TT_VAR, None, *self._q(q))

    def conv(self, cout, k=1, pad=0, group=1, src=None):
        g, rng, dt = self.g, self.rng, self.dtype
        x = self.cur if src is None else src
        n, cin, h, w = self.dims(x)
        name = self._name("conv")
        fan = (cin // group) * k * k
        shape = (cout, cin // group, k, k)
        if dt == DT_FP32:
            ins = [x, g.add_const(name + "_w", rng.normal(0, 1 / np.sqrt(fan), size=shape), DT_FP32),
                   g.add_const(name + "_b", rng.normal(0, 0.1, size=(cout,)), DT_FP32)]
            q = None
        elif dt == DT_INT8:
            xs = self.scale(x)
            ws = [f32(v) for v in rng.uniform(0.002, 0.02, size=cout)]
            ins = [x, g.add_const(name + "_w", rng.integers(-127, 128, size=shape), DT_INT8, ws, [0] * cout),
                   g.add_const(name + "_b", rng.integers(-2000, 2000, size=(cout,)), DT_INT32, [1.0], [0])]
            q = (xs * np.mean(ws) * 73.0 * np.sqrt(fan) * 73.0 / 60.0, 0)
        else:
            xs = self.scale(x)
            ws, wz = f32(rng.uniform(0.002, 0.02)), int(rng.integers(112, 144))
            ins = [x, g.add_const(name + "_w", rng.integers(0, 256, size=shape), DT_UINT8, [ws], [wz]),
                   g.add_const(name + "_b", rng.integers(-4000, 4000, size=(cout,)), DT_INT32, [f32(np.float32(xs) * np.float32(ws))], [0])]
            q = (xs * ws * 73.0 * np.sqrt(fan) * 73.0 / 40.0, int(rng.integers(100, 156)))
        oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
        y = self._var(name, [n, cout, oh, ow], q)
        self.last = g.add_node(name, "Convolution", ins, [y], kernel_h=k, kernel_w=k, stride_h=1, stride_w=1, dilation_h=1, dilation_w=1,
                               input_channel=cin, output_channel=cout, group=group, activation=-1, pad_h0=pad, pad_w0=pad, pad_h1=pad, pad_w1=pad)
        self.cur = y
        return y

    def fc(self, nout):
        g, rng = self.g, self.rng
        assert self.dtype == DT_INT8
        d = self.dims()
        hidden = int(np.prod(d[1:]))
        ws = [f32(v) for v in rng.uniform(0.002, 0.02, size=nout)]
        ins = [self.cur, g.add_const("fc_w", rng.integers(-127, 128, size=(nout, hidden)), DT_INT8, ws, [0] * nout),
               g.add_const("fc_b", rng.integers(-2000, 2000, size=(nout,)), DT_INT32, [1.0], [0])]
        y = self._var("fc", [d[0], nout], (self.scale() * np.mean(ws) * 73.0 * np.sqrt(hidden) * 73.0 / 60.0, 0))
        self.last = g.add_node("fc", "FullyConnected", ins, [y], num_output=nout)
        self.cur = y
        return y

    def act(self, op, out_q=None, params=None):
        """out_q None: a range that fits the operator (Sigmoid (0, 1); Clip its bounds; HardSwish / Mish the input's range)"""
        p = DEFAULT_PARAMS[op] if params is None else params
        if out_q is None and self.dtype != DT_FP32:
            if op == "Sigmoid":
                out_q = (1 / 127.0, 0) if self.dtype == DT_INT8 else (1 / 255.0, 0)
            elif op == "Clip":
                out_q = (p["max"] / 127.0, 0) if self.dtype == DT_INT8 else ((p["max"] - p["min"]) / 255.0, int(round(-p["min"] / ((p["max"] - p["min"]) / 255.0))))
            else:
                out_q = (self.scale() * 0.6, 30)
        name = self._name(op.lower())
        y = self._var(name, self.dims(), out_q)
        self.last = self.g.add_node(name, op, [self.cur], [y], **p)
        self.cur = y
        return y

    def reshape(self, dims, re_shape):
        """a Reshape (same quantisation): its result is dense on the device in an int8 graph"""
        t = self.g.tensors[self.cur]
        y = self._var("rs", dims, None if self.dtype == DT_FP32 else (t.scales[0], t.zero_points[0]))
        self.last = self.g.add_node("rs", "Reshape", [self.cur], [y], is_mxnet=0, reverse=0, is_onnx=1, re_shape=list(re_shape))
        self.cur = y
        return y

    def prod(self, a, b):
        name = self._name("prod")
        q = None if self.dtype == DT_FP32 else (self.scale(a) * 0.5, 0 if self.dtype == DT_INT8 else 128)
        y = self._var(name, self.dims(a), q)
        self.last = self.g.add_node(name, "Eltwise", [a, b], [y], type=tm2.ELT_PROD, caffe_flavor=1)
        self.cur = y
        return y

    def maxpool(self):
        n, c, h, w = self.dims()
        name = self._name("pool")
        t = self.g.tensors[self.cur]
        y = self._var(name, [n, c, h // 2, w // 2], None if self.dtype == DT_FP32 else (t.scales[0], t.zero_points[0]))
        self.last = self.g.add_node(name, "Pooling", [self.cur], [y], alg=0, kernel_h=2, kernel_w=2, stride_h=2, stride_w=2, **{"global": 0},
                                    caffe_flavor=0, pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
        self.cur = y
        return y

    def done(self, seed=1):
        self.g.output_nodes = [self.last]
        d = self.g.tensors[self.g.nodes[self.g.input_nodes[0]].outputs[0]].dims
        if self.dtype == DT_FP32:
            return self.g, np.random.default_rng(seed).normal(0, 1, size=d).astype(np.float32)
        return self.g, random_bytes(seed, self.dtype, d) if self.dtype == DT_UINT8 else np.random.default_rng(seed).integers(-127, 128, size=d).astype(np.int8)


def placement_a(dtype, dims=(1, 8, 6, 6)):
    """conv -> Clip(0, 6) -> conv -> Sigmoid"""
    c = Chain(21, dtype, dims)
    c.conv(16, 3, 1); c.act("Clip"); c.conv(12, 1); c.act("Sigmoid")
    return c.done()


def placement_b(dtype, dims=(1, 8, 6, 6)):
    """conv -> Mish -> conv -> HardSwish"""
    c = Chain(22, dtype, dims)
    c.conv(16, 3, 1); c.act("Mish"); c.conv(12, 1); c.act("HardSwish")
    return c.done()


def silu_graph(dims=(2, 8, 5, 3), cout=16):
    """int8 conv -> Sigmoid -> Eltwise PROD(conv, sigmoid): the activation of YOLOX / YOLOv5"""
    c = Chain(23, DT_INT8, dims)
    a = c.conv(cout, 3, 1)
    s = c.act("Sigmoid")
    c.prod(a, s)
    return c.done()


def relu6_block_graph(dims=(1, 8, 7, 5)):
    """int8 conv -> Clip(0, 6) -> depthwise 3x3 -> Clip(0, 6) -> conv: a MobileNet-v2 block as ONNX exports it"""
    c = Chain(24, DT_INT8, dims)
    c.conv(16, 1); c.act("Clip"); c.conv(16, 3, 1, group=16); c.act("Clip"); c.conv(8, 1)
    return c.done()


def mish_pool_graph(dims=(1, 4, 8, 8)):
    """uint8 conv -> Mish -> 2x2 max-pool: a YOLOv4-tiny stage"""
    c = Chain(25, DT_UINT8, dims)
    c.conv(8, 3, 1); c.act("Mish"); c.maxpool()
    return c.done()


def padding_graph(op, dims=(2, 8, 5, 3)):
    """int8 conv1x1 (8 -> 5) -> op -> conv3x3 pad 1 (5 -> 7): the 5-channel tensors have 11 padding lanes per pixel on the device, and
    the second convolution's K loop reads them"""
    c = Chain(26, DT_INT8, dims)
    c.conv(5, 1); c.act(op); c.conv(7, 3, 1)
    return c.done()


def fc_sigmoid_graph():
    """int8 FC(2 x 40 -> 10) -> Sigmoid"""
    c = Chain(27, DT_INT8, (2, 40))
    c.fc(10); c.act("Sigmoid")
    return c.done()


def dense_graph(op, n=2, c=5, h=3, w=7):
    """int8 conv (-> 5 channels) -> Reshape [n, c * h, w] -> op: the Reshape's result is in the reference's dense element order on the
    device (c * h * w = 105 bytes per image: no padding lanes, a ragged last vector)"""
    ch = Chain(28, DT_INT8, (n, 8, h, w))
    ch.conv(c, 1); ch.reshape([n, c * h, w], [0, -1, w]); ch.act(op)
    return ch.done()


class TensorDesc(C.Structure):          # tamd_tensor_desc
    _fields_ = [("dtype", C.c_int), ("ttype", C.c_int), ("dim_num", C.c_int), ("dims", C.c_int * 8), ("data", C.c_void_p),
                ("quant_num", C.c_int), ("scales", C.c_void_p), ("zero_points", C.c_void_p), ("name", C.c_char_p)]


class NodeDesc(C.Structure):            # tamd_node_desc
    _fields_ = [("op", C.c_int), ("input_num", C.c_int), ("inputs", C.c_void_p), ("output_num", C.c_int), ("outputs", C.c_void_p),
                ("param", C.c_void_p), ("name", C.c_char_p)]


def ask_node(capi, op, dtype, dims, with_param=True):
    """tamd_node_supported for one of the four operators on a tensor of `dims`"""
    def t():
        d = TensorDesc()
        d.dtype, d.ttype, d.dim_num, d.quant_num = dtype, 1, len(dims), 0 if dtype == DT_FP32 else 1
        for i, v in enumerate(dims):
            d.dims[i] = v
        return d
    n = NodeDesc()
    n.op, n.input_num, n.output_num = OPCODE[op], 1, 1
    p = (C.c_float * 2)(6.0, 0.0)
    if with_param and op in ("Clip", "HardSwish"):
        n.param = C.cast(p, C.c_void_p)
    return capi.lib().tamd_node_supported(C.byref(n), (TensorDesc * 1)(t()), 1, (TensorDesc * 1)(t()), 1)
