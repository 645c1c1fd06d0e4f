"""Builders for the tests of the quantised PReLU node (tests/test_prelu_cpu.py, tests/test_gpu_prelu.py, tools/make_golden_prelu.py):
single-node graphs with chosen quantisation parameters and fp16 slope bit patterns, the slope set that reaches every branch of the
reference's kernels and of its half-widening routine, and the MobileFaceNet bottleneck.  Every case is tmfile bytes: the reference
library and the device read the same model."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP16, DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prelu_cases.npz")
OP_PRELU = 25            # TAMD_OP_PRELU
f32 = lh.f32
equals_golden = ih.equals_golden


def half(v):
    """the bit pattern of the fp16 nearest to v"""
    return int(np.array([v], np.float16).view(np.uint16)[0])


# (what it is for, fp16 bit pattern).  The reference widens the slopes with its own routine (source/utility/float.c), in which a normal
# half whose fraction is zero -- every exact power of two -- comes out as +0
SLOPES = [
    ("quarter_acts_as_0", 0x3400),       # 0.25, the customary initial slope: a ReLU in the reference
    ("zero", 0x0000),
    ("tenth", half(0.1)),
    ("negative", half(-0.3)),            # negative inputs come out positive
    ("four_acts_as_0", 0x4400),          # 4.0
    ("saturates", half(3.3)),            # with the output scales below, the negative side passes the end of the range
    ("subnormal", 0x0003),               # widened to 0x34000200 (1.19e-7), not 2^-24 * 3
    ("minus_zero", 0x8000),
]
SLOPE_BITS = [b for _, b in SLOPES]
ALL_BYTES_C = (5, 16, 20)               # int8 on the device: 11 padding lanes; none; a second, quarter-full 16-lane group


def slopes_for(c, first=0):
    """c slope bit patterns, the set above in turn"""
    return [SLOPE_BITS[(first + i) % len(SLOPE_BITS)] for i in range(c)]


def slope_const(g, name, bits):
    return g.add_const(name, np.array(bits, np.uint16).view(np.float16), DT_FP16)


def unary_graph(dtype, dims, in_q, out_q, bits, slope_dtype=DT_FP16):
    """input(dims) -> PReLU(slope: the fp16 constant with these bit patterns) -> output; in_q / out_q: (scale, zero point)"""
    g = Graph(name="prelu_case")
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    if slope_dtype == DT_FP16:
        s = slope_const(g, "slope", bits)
    else:
        s = g.add_const("slope", np.array(bits, np.uint16).view(np.float16).astype(np.float32), slope_dtype)
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, *q(out_q))
    g.output_nodes = [g.add_node("prelu", "PReLU", [x, s], [y])]
    return g


def all_bytes(dtype, c):
    """(1, c, 16, 16): every channel holds every byte value, element i of a plane the value i"""
    return np.tile(np.arange(256, dtype=np.uint8), c).view(lh.NP[dtype]).reshape(1, c, 16, 16)


# (id, type, C, (in scale, in zp), (out scale, out zp), shared slope bits or None).  int8: 0.05 in, 0.031 out -- 127 * 0.05 / 0.031 = 205
# saturates at +127, -128 * 0.05 * 3.3 / 0.031 = -681 at -127, and -128 is among the inputs.  uint8: the input zero point at both ends
# and in the middle, the output's another one; 0.02 out saturates both ends for the slope 3.3
ALL_BYTES_SETS = [("i8_c%d" % c, DT_INT8, c, (0.05, 0), (0.031, 0), None) for c in ALL_BYTES_C] + [
    ("u8_c5_zp0", DT_UINT8, 5, (0.05, 0), (0.031, 12), None),
    ("u8_c16_zp128", DT_UINT8, 16, (0.05, 128), (0.02, 100), None),
    ("u8_c20_zp255", DT_UINT8, 20, (0.05, 255), (0.031, 200), None),
    ("u8_c5_shared_tenth", DT_UINT8, 5, (0.05, 128), (0.031, 77), half(0.1)),
    ("u8_c16_shared_quarter", DT_UINT8, 16, (0.05, 100), (0.031, 128), 0x3400),
]


def all_bytes_case(case):
    """-> (graph, input, [slope bits of every channel])"""
    _, dtype, c, in_q, out_q, shared = case
    bits = slopes_for(c) if shared is None else [shared]
    return unary_graph(dtype, (1, c, 16, 16), in_q, out_q, bits), all_bytes(dtype, c), bits * (1 if shared is None else c)


def tables_of(dtype, bits, in_q, out_q):
    """[C, 256]: tamd_prelu_table of every channel"""
    return np.stack([capi.prelu_table(dtype, b, f32(in_q[0]), int(in_q[1]), f32(out_q[0]), int(out_q[1])) for b in bits])


def expected_all_bytes(case):
    """what tamd_prelu_table says the all-bytes graph gives: (1, C, 16, 16)"""
    _, dtype, c, in_q, out_q, shared = case
    bits = slopes_for(c) if shared is None else [shared] * c
    return tables_of(dtype, bits, in_q, out_q).view(lh.NP[dtype]).reshape(1, c, 16, 16)


class Face(ih.Neck):
    """interp_helpers.Neck with PReLU and the residual sum"""

    def prelu(self, bits=None, out_q=None, src=None):
        """bits None: a trained-looking slope per channel (0.05 .. 0.4), with 0.25 -- which acts as 0 -- on channel 0"""
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("prelu")
        if bits is None:
            bits = [0x3400] + [half(v) for v in self.rng.uniform(0.05, 0.4, size=c - 1)]
        if out_q is None:
            out_q = (self.scale(x) * 0.8, 0 if self.dtype == DT_INT8 else 40)
        y = self._var(name, [n, c, h, w], out_q)
        self.last = self.g.add_node(name, "PReLU", [x, slope_const(self.g, name + "_slope", bits)], [y])
        self.cur = y
        return y

    def add(self, a, b):
        name = self._name("sum")
        q = None if self.dtype == DT_FP32 else (max(self.scale(a), self.scale(b)) * 1.5, 0 if self.dtype == DT_INT8 else 128)
        y = self._var(name, self.dims(a), q)
        self.last = self.g.add_node(name, "Eltwise", [a, b], [y], type=tm2.ELT_SUM, caffe_flavor=1)
        self.cur = y
        return y


def geometry_graph(dtype, dims, seed):
    """one PReLU node on random bytes (every value, -128 included), a slope per channel from the set above"""
    in_q, out_q = ((0.05, 0), (0.031, 0)) if dtype == DT_INT8 else ((0.05, 77), (0.031, 12))
    return unary_graph(dtype, dims, in_q, out_q, slopes_for(dims[1], first=seed)), lh.random_bytes(seed, dtype, dims)


def shared_geometry_graph(dims=(2, 3, 7, 7), seed=9):
    """uint8, one slope for all channels"""
    return unary_graph(DT_UINT8, dims, (0.05, 77), (0.031, 12), [half(0.1)]), lh.random_bytes(seed, DT_UINT8, dims)


def padding_graph(dims=(2, 8, 5, 3)):
    """int8 conv1x1 (8 -> 5) -> PReLU -> conv3x3 pad 1 (5 -> 7), after lut_helpers.padding_graph: the 5-channel tensors have 11 padding
    lanes per pixel on the device, and the second convolution's K loop reads the lanes the PReLU must have zeroed"""
    c = Face(51, DT_INT8, dims)
    c.conv(5, 1); c.prelu(); c.conv(7, 3, 1)
    return c.done()


def bottleneck_graph(dtype, dims=(1, 8, 8, 8), mid=16):
    """the MobileFaceNet bottleneck: conv1x1 -> PReLU -> depthwise 3x3 -> PReLU -> conv1x1 (linear), plus an Eltwise SUM with the block's
    input.  In an fp32 graph the slopes are fp32 constants, as the converters write them"""
    c = Face(52, dtype, dims)
    data = c.cur
    if dtype == DT_FP32:
        return _bottleneck_fp32(c, data, mid)
    c.conv(mid, 1); c.prelu(); c.conv(mid, 3, 1, group=mid); c.prelu()
    y = c.conv(dims[1], 1)
    c.add(data, y)
    return c.done()


def _bottleneck_fp32(c, data, mid):
    def prelu():
        x = c.cur
        name = c._name("prelu")
        y = c._var(name, c.dims(x), None)
        s = c.g.add_const(name + "_slope", c.rng.uniform(0.05, 0.4, size=c.dims(x)[1]), DT_FP32)
        c.last = c.g.add_node(name, "PReLU", [x, s], [y])
        c.cur = y
    c.conv(mid, 1); prelu(); c.conv(mid, 3, 1, group=mid); prelu()
    y = c.conv(c.dims(data)[1], 1)
    c.add(data, y)
    return c.done()


def quarter_and_relu_graphs(dtype, dims=(1, 5, 6, 7), seed=11):
    """the same input through PReLU(0.25 on every channel) and through ReLU, equal quantisation: equal bytes in the reference"""
    in_q, out_q = ((0.05, 0), (0.031, 0)) if dtype == DT_INT8 else ((0.05, 77), (0.031, 12))
    gp = unary_graph(dtype, dims, in_q, out_q, [0x3400] * dims[1])
    gr = Graph(name="relu_case")
    x = gr.add_input("data", list(dims), dtype, [f32(in_q[0])], [in_q[1]])
    y = gr.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, [f32(out_q[0])], [out_q[1]])
    gr.output_nodes = [gr.add_node("relu", "ReLU", [x], [y], negative_slope=0.0)]
    return gp, gr, lh.random_bytes(seed, dtype, dims)


def gpu_cases():
    """{id: (dtype, builder)}: every graph the GPU tests run against the reference; a builder returns (graph, input)"""
    I8, U8 = DT_INT8, DT_UINT8
    cases = {}
    for s in ALL_BYTES_SETS:
        cases["all_bytes_" + s[0]] = (s[1], lambda s=s: all_bytes_case(s)[:2])
    cases.update({
        "u8_planes_49_bytes_batch2": (U8, lambda: geometry_graph(U8, (2, 3, 7, 7), 1)),
        "u8_planes_1_byte": (U8, lambda: geometry_graph(U8, (1, 2, 1, 1), 2)),
        "u8_plane_335_bytes": (U8, lambda: geometry_graph(U8, (1, 1, 5, 67), 3)),
        "u8_planes_aligned": (U8, lambda: geometry_graph(U8, (2, 4, 4, 4), 4)),
        "u8_planes_shared_slope": (U8, shared_geometry_graph),
        "i8_batch2_minus128": (I8, lambda: geometry_graph(I8, (2, 20, 5, 3), 5)),
        "i8_padding": (I8, padding_graph),
        "i8_bottleneck": (I8, lambda: bottleneck_graph(I8)),
        "u8_bottleneck": (U8, lambda: bottleneck_graph(U8)),
    })
    return cases


def reference_outputs(ref, g, x, dtype):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


def golden():
    return np.load(GOLDEN)


def golden_entry(case, x, outs):
    """the case's input and the reference's outputs"""
    e = {case + "__n": np.int32(len(outs)), case + "__in": x}
    for i, o in enumerate(outs):
        e["%s__out%d" % (case, i)] = o
    return e


def library_error(tm_bytes):
    """the error prerun leaves.  Shape inference and validation run before tamd_graph_prerun touches the device, so this answers
    without a GPU too"""
    return ih.library_output_shape(capi, tm_bytes)[1]


def _desc(dtype, dims, ttype=1, quant=None, data=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype in (DT_FP32, DT_FP16) else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    if data is not None:
        d.data = data.ctypes.data_as(C.c_void_p)
    return d


def ask_node(dtype, dims, bits, slope_dtype=DT_FP16, slope_const_=True, const_input=False, in_quant=None, out_quant=None, with_payload=True, inputs=2):
    """tamd_node_supported for a PReLU node on a tensor of `dims` with these slope bit patterns"""
    payload = np.array(bits, np.uint16)
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_PRELU, inputs, 1
    ins = (lh.TensorDesc * 2)(_desc(dtype, dims, 2 if const_input else 1, in_quant),
                              _desc(slope_dtype, [len(bits)], 2 if slope_const_ else 1, data=payload if with_payload else None))
    return capi.lib().tamd_node_supported(C.byref(n), ins, inputs, (lh.TensorDesc * 1)(_desc(dtype, dims, quant=out_quant)), 1)
