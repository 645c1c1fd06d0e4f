"""Builders for the tests of the channel-gate Eltwise -- x (N, C, H, W) op gate (N, C, 1, 1), the last node of a Squeeze-and-Excitation
block -- (tests/test_se_cpu.py, tests/test_gpu_se.py, tools/make_golden_se.py): two-input graphs with chosen quantisation parameters,
the all-byte-pairs inputs, the numpy restatement of what the reference computes, and whole SE blocks.  Every case is tmfile bytes: the
reference library and the device read the same model.  A case's inputs are a LIST (the two-input graphs have two)."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, ELT_MAX, ELT_PROD, ELT_SUB, ELT_SUM, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "se_cases.npz")
OP_ELTWISE = 6           # TAMD_OP_ELTWISE
f32 = lh.f32
TYPES = {"prod": ELT_PROD, "sum": ELT_SUM, "sub": ELT_SUB}

# (x (scale, zp), gate (scale, zp), {type: output (scale, zp)}).  Both ends of the output range are passed in all six:
# int8: x * 0.05 in [-6.4, 6.35], gate * 0.02 in [-2.56, 2.54]: the product reaches +-16.4 = +-164 steps of 0.1, sums and differences
#   +-8.9 = +-179 steps of 0.05.
# uint8: x in [-5, 7.75], gate in [-2.8, 2.3]: the product spans [-21.7, 17.8] = [-217, 178] steps of 0.1 around zero point 128, the
#   sum [-7.8, 10.05] and the difference [-7.3, 10.55] = [-156, 211] steps of 0.05.
QUANT = {
    DT_INT8: ((0.05, 0), (0.02, 0), {"prod": (0.1, 0), "sum": (0.05, 0), "sub": (0.05, 0)}),
    DT_UINT8: ((0.05, 100), (0.02, 140), {"prod": (0.1, 128), "sum": (0.05, 128), "sub": (0.05, 128)}),
}


def gate_graph(dtype, typ, x_dims, g_dims, gate_first=False, out_q=None, qx=None, qg=None, const_gate=False):
    """inputs x (x_dims) and gate (g_dims) -> Eltwise(type) -> output with the dims of the operand with more elements.  gate_first: the
    node lists the gate as input 0.  typ: a key of TYPES or an eltwise type number"""
    name = typ if isinstance(typ, str) else "t%d" % typ
    code = TYPES[typ] if isinstance(typ, str) else typ
    g = Graph(name="se_gate_case")
    dx, dg, do = QUANT.get(dtype, (None, None, {}))
    qx, qg = qx or dx, qg or dg
    out_q = out_q or do.get(name, (0.05, 0 if dtype == DT_INT8 else 128))
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(x_dims), dtype, *q(qx))
    if const_gate:
        gt = g.add_const("gate", np.ones(g_dims, lh.NP[dtype]), dtype, *q(qg))
    else:
        gt = g.add_input("gate", list(g_dims), dtype, *q(qg))
    big = x_dims if np.prod(x_dims) >= np.prod(g_dims) else g_dims
    y = g.add_tensor("out", list(big), dtype, tm2.TT_VAR, None, *q(out_q))
    g.output_nodes = [g.add_node("gate_" + name, "Eltwise", [gt, x] if gate_first else [x, gt], [y], type=code, caffe_flavor=1)]
    return g


def all_pairs_inputs(dtype):
    """x (1, 256, 16, 16): every channel holds all 256 byte values; gate (1, 256, 1, 1): byte c in channel c -- all 65 536 pairs"""
    x = np.tile(np.arange(256, dtype=np.uint8), 256).view(lh.NP[dtype]).reshape(1, 256, 16, 16)
    gate = np.arange(256, dtype=np.uint8).view(lh.NP[dtype]).reshape(1, 256, 1, 1)
    return [x, gate]


def all_pairs_case(dtype, typ):
    return gate_graph(dtype, typ, (1, 256, 16, 16), (1, 256, 1, 1)), all_pairs_inputs(dtype)


def restate(dtype, typ, x, gate, qx, qg, qo):
    """what eltwise_ref.c computes for x (N, C, H, W) op gate (N, C, 1, 1), in numpy: both operands dequantised in float32, the
    operation in float32, round(f / out_scale) -- C round on the float quotient: half away from zero -- (+ the zero point), clamped"""
    sx, sg, so = np.float32(qx[0]), np.float32(qg[0]), np.float32(qo[0])
    if dtype == DT_INT8:
        fx, fg = x.astype(np.float32) * sx, gate.astype(np.float32) * sg
    else:
        fx = (x.astype(np.int32) - int(qx[1])).astype(np.float32) * sx
        fg = (gate.astype(np.int32) - int(qg[1])).astype(np.float32) * sg
    f = {"prod": fx * fg, "sum": fx + fg, "sub": fx - fg}[typ].astype(np.float32)
    d = (f / so).astype(np.float32).astype(np.float64)
    r = (np.sign(d) * np.floor(np.abs(d) + 0.5)).astype(np.int64)
    if dtype == DT_INT8:
        return np.clip(r, -127, 127).astype(np.int8)
    return np.clip(r + int(qo[1]), 0, 255).astype(np.uint8)


def random_inputs(seed, dtype, x_dims, g_dims, force=None):
    """every byte value; force: a value that is put into both operands several times (-128)"""
    x, gate = lh.random_bytes(seed, dtype, x_dims), lh.random_bytes(seed + 100, dtype, g_dims)
    if force is not None:
        x.reshape(-1)[:: max(1, x.size // 7)] = force
        gate.reshape(-1)[:: max(1, gate.size // 3)] = force
    return [x, gate]


def geometry_case(dtype, typ, dims, seed, gate_first=False):
    g_dims = (dims[0], dims[1], 1, 1)
    return gate_graph(dtype, typ, dims, g_dims, gate_first=gate_first), random_inputs(seed, dtype, dims, g_dims, force=-128 if dtype == DT_INT8 else None)


class Block(ih.Neck):
    """interp_helpers.Neck with the nodes of a Squeeze-and-Excitation block"""

    def gap(self, src=None):
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("gap")
        y = self._var(name, [n, c, 1, 1], self.quant(x))
        self.last = self.g.add_node(name, "Pooling", [x], [y], alg=1, kernel_h=h, kernel_w=w, stride_h=1, stride_w=1, **{"global": 1},
                                    caffe_flavor=0, pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
        self.cur = y
        return y

    def relu(self):
        name = self._name("relu")
        y = self._var(name, self.dims(), self.quant(self.cur))
        self.last = self.g.add_node(name, "ReLU", [self.cur], [y], negative_slope=0.0)
        self.cur = y
        return y

    def gate(self, x, gt, typ="prod", gate_first=False, out_q=None):
        name = self._name(typ)
        q = None if self.dtype == DT_FP32 else (out_q or (self.scale(x) * (0.6 if typ == "prod" else 1.2), 0 if self.dtype == DT_INT8 else 120))
        y = self._var(name, self.dims(x), q)
        code = TYPES[typ] if typ in TYPES else ELT_MAX
        self.last = self.g.add_node(name, "Eltwise", [gt, x] if gate_first else [x, gt], [y], type=code, caffe_flavor=1)
        self.cur = y
        return y


def se_block_graph(dtype, dims=(2, 8, 6, 6), reduce=4, typ="prod", act="Sigmoid", mid=None, seed=61, k=3):
    """conv k x k -> [global average pool -> conv 1x1 (C -> reduce) -> ReLU -> conv 1x1 (reduce -> C) -> Sigmoid] -> Eltwise PROD(conv, gate) -> conv 1x1"""
    c = Block(seed, dtype, dims)
    mid = mid or dims[1]
    x = c.conv(mid, k, k // 2)
    c.gap()
    c.conv(reduce, 1); c.relu(); c.conv(mid, 1)
    gt = c.act(act)
    c.gate(x, gt, typ)
    c.conv(dims[1], 1)
    return c.done()


def padding_graph(dims=(2, 8, 5, 3)):
    """int8 conv 1x1 (8 -> 5) -> SUM with a gate (global average pool of it) -> conv 3x3 pad 1 (5 -> 7): the 5-channel tensors have 11
    padding lanes per pixel on the device, and the second convolution's K loop reads the lanes the gate kernel must have zeroed"""
    c = Block(62, DT_INT8, dims)
    x = c.conv(5, 1)
    gt = c.gap()
    c.gate(x, gt, "sum")
    c.conv(7, 3, 1)
    return c.done()


def multi_reader_graph(dtype, dims=(2, 8, 6, 6)):
    """the SE block whose Sigmoid output is ALSO a graph output: the byte map cannot be folded into the gate's launch"""
    c = Block(63, dtype, dims)
    x = c.conv(dims[1], 3, 1)
    c.gap(); c.conv(4, 1); c.relu(); c.conv(dims[1], 1)
    gt = c.act("Sigmoid")
    sig_node = c.last
    c.gate(x, gt, "prod")
    g, xin = c.done()
    g.output_nodes = [c.last, sig_node]
    return g, xin


def _one(gx):
    g, x = gx
    return g, [x]


def gpu_cases():
    """{id: (dtype, builder)}: every graph the GPU tests run against the reference; a builder returns (graph, [inputs])"""
    I8, U8 = DT_INT8, DT_UINT8
    cases = {}
    for dt, tag in ((I8, "i8"), (U8, "u8")):
        for typ in TYPES:
            cases["pairs_%s_%s" % (tag, typ)] = (dt, lambda dt=dt, typ=typ: all_pairs_case(dt, typ))
        cases["%s_se_block" % tag] = (dt, lambda dt=dt: _one(se_block_graph(dt)))
        cases["%s_multi_reader" % tag] = (dt, lambda dt=dt: _one(multi_reader_graph(dt)))
        for typ in TYPES:
            cases["%s_gate_first_%s" % (tag, typ)] = (dt, lambda dt=dt, typ=typ: geometry_case(dt, typ, (1, 5, 3, 3), 7, gate_first=True))
    for k, (c, typ) in enumerate(((5, "prod"), (16, "sum"), (20, "sub"))):          # int8 lane geometry: 11 padding lanes; none; a second, quarter-full group
        cases["i8_lanes_c%d" % c] = (I8, lambda c=c, typ=typ, k=k: geometry_case(I8, typ, (2, c, 3, 3), 11 + k))
    cases["i8_walk_c480"] = (I8, lambda: geometry_case(I8, "prod", (2, 480, 5, 5), 14))       # 30 groups: 8 pixels per block iteration, 25 pixels
    cases["i8_two_pixels"] = (I8, lambda: geometry_case(I8, "prod", (1, 16, 1, 2), 15))
    cases["i8_padding"] = (I8, lambda: _one(padding_graph()))
    cases["u8_planes_49_bytes_batch2"] = (U8, lambda: geometry_case(U8, "prod", (2, 3, 7, 7), 21))
    cases["u8_planes_2_bytes"] = (U8, lambda: geometry_case(U8, "sum", (1, 2, 1, 2), 22))
    cases["u8_planes_335_bytes"] = (U8, lambda: geometry_case(U8, "sub", (1, 2, 5, 67), 23))
    cases["u8_planes_aligned"] = (U8, lambda: geometry_case(U8, "prod", (2, 4, 4, 4), 24))
    return cases


def reference_outputs(ref, g, xs, dtype, tm_bytes=None):
    """the outputs of the real reference library on its CPU device; raises RuntimeError where its run_graph fails"""
    rg = ref.RefGraph(tm_bytes or tm2.write_tm2(g), lh.ref_mode(ref, dtype), 1)
    for i, x in enumerate(xs):
        rg.set_input(x, i)
    try:
        rg.run()
        return rg.outputs()
    finally:
        rg.close()


def device_outputs(tm_bytes, xs, **kw):
    """through the C ABI: run, the launch list's kernel names, run again (the launches are idempotent) -> (outputs, names, halves); a graph
    compiled as two half-batch graphs (split_batch) has no launch list of its own: names is empty"""
    gr = capi.Graph(tm_bytes, **kw)
    for i, x in enumerate(xs):
        gr.set_input(x, i)
    out = gr.run()
    names = [] if gr.halves() else [k["kernel"] for k in gr.profile(1)]
    again = gr.run()
    halves = gr.halves()
    gr.close()
    for a, c in zip(out, again):
        assert np.array_equal(a, c)
    return out, names, halves


def child_main(case, path):
    """what a fresh child process runs for the GPU tests (python -c ...: the environment it was started with decides the plan): the case
    through the C ABI, its outputs and kernel names saved to `path`"""
    dtype, build = gpu_cases()[case]
    g, xs = build()
    out, names, _ = device_outputs(tm2.write_tm2(g), xs)
    np.savez(path, names=np.array(names), **{"out%d" % i: o for i, o in enumerate(out)})


def golden():
    return np.load(GOLDEN)


equals_golden = ih.equals_golden


def golden_entry(case, xs, outs):
    """the case's inputs and the reference's outputs"""
    e = {case + "__n": np.int32(len(outs)), case + "__nin": np.int32(len(xs))}
    for i, x in enumerate(xs):
        e["%s__in%d" % (case, i)] = x
    for i, o in enumerate(outs):
        e["%s__out%d" % (case, i)] = o
    return e


def library_output_shape(tm_bytes):
    """(the shape the library infers for output 0, the error prerun leaves).  Shape inference and validation run before
    tamd_graph_prerun touches the device, so this answers without a GPU too"""
    return ih.library_output_shape(capi, tm_bytes)


def library_error(tm_bytes):
    return library_output_shape(tm_bytes)[1]


class EltwiseParam(C.Structure):        # tamd_eltwise_param
    _fields_ = [("type", C.c_int), ("caffe_flavor", C.c_int), ("shift", C.c_float), ("power", C.c_float), ("scale", C.c_float)]


def _desc(dtype, dims, ttype=1, quant=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == DT_FP32 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def ask_node(dtype, typ, a_dims, b_dims, out_dims=None, a_const=False, b_const=False, a_quant=None, b_quant=None, out_quant=None, with_param=True):
    """tamd_node_supported for an Eltwise node with inputs of dims a_dims, b_dims; out_dims None: those of the operand with more elements"""
    if out_dims is None:
        out_dims = a_dims if np.prod(a_dims) >= np.prod(b_dims) else b_dims
    p = EltwiseParam(typ, 1, 0.0, 1.0, 1.0)
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_ELTWISE, 2, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    ins = (lh.TensorDesc * 2)(_desc(dtype, a_dims, 2 if a_const else 1, a_quant), _desc(dtype, b_dims, 2 if b_const else 1, b_quant))
    return capi.lib().tamd_node_supported(C.byref(n), ins, 2, (lh.TensorDesc * 1)(_desc(dtype, out_dims, quant=out_quant)), 1)
