"""Builders for the tests of the quantised Split and ShuffleChannel nodes (tests/test_shuffle_cpu.py, tests/test_gpu_shuffle.py,
tools/make_golden_shuffle.py): single-node graphs with chosen quantisation parameters, and the ShuffleNet-v2 units around them --
Split -> (1x1 -> dw3x3 -> 1x1) -> Concat -> ShuffleChannel.  Every case is tmfile bytes with explicit quantisation parameters: the
reference library and the device read the same model.

A Split alone as an output node shows only its output 0 through RefGraph.outputs(), so the single-node Split cases are
data -> Split -> Concat(the outputs in reverse order)."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shuffle_cases.npz")
OP_SPLIT, OP_SHUFFLECHANNEL = 22, 23          # TAMD_OP_*
f32 = lh.f32
digest, equals_golden = ih.digest, ih.equals_golden
DIGEST_ONLY = {"i8_shuffle_ragged_blocks"}    # ~24 KB of random bytes: the golden holds their shape and SHA-256


class Unit(ih.Neck):
    """interp_helpers.Neck with the two channel movers"""

    def split(self, sizes, out_qs=None, src=None, **kw):
        """-> the output tensors; out_qs: one (scale, zero point) per output, None: the input's"""
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("split")
        outs = [self._var("%s_%d" % (name, i), [n, s, h, w], self.quant(x) if out_qs is None else out_qs[i]) for i, s in enumerate(sizes)]
        self.last = self.g.add_node(name, "Split", [x], outs, axis=1, split_sizes=list(sizes), **kw)
        self.cur = outs[0]
        return outs

    def shuffle(self, group, out_q=None, src=None):
        x = self.cur if src is None else src
        name = self._name("shuffle")
        y = self._var(name, self.dims(x), self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "ShuffleChannel", [x], [y], group=group)
        self.cur = y
        return y

    def branch(self, half, src, q):
        """1x1 -> depthwise 3x3 -> 1x1, the last one at quantisation q (the Concat's, so that the reference's concat is a copy)"""
        self.conv(half, 1, src=src); self.conv(half, 3, 1, group=half); y = self.conv(half, 1)
        self.requant(y, q)
        return y

    def basic_unit(self, half):
        """Split [half, half] -> (x1, branch(x2)) -> Concat -> ShuffleChannel(2)"""
        x1, x2 = self.split([half, half])
        q = self.quant(x1)
        self.concat([x1, self.branch(half, x2, q)], q)
        return self.shuffle(2)

    def down_unit(self, half):
        """two branches of the same tensor (depthwise 3x3 -> 1x1 | 1x1 -> depthwise 3x3 -> 1x1) -> Concat -> ShuffleChannel(2)"""
        x = self.cur
        c = self.dims(x)[1]
        q = self.quant(x)
        self.conv(c, 3, 1, group=c, src=x); a = self.conv(half, 1)
        self.requant(a, q)
        self.concat([a, self.branch(half, x, q)], q)
        return self.shuffle(2)


def _bytes(seed, dtype, dims, force=None):
    x = lh.random_bytes(seed, dtype, dims)
    if force is not None:
        x.reshape(-1)[:: max(1, x.size // 7)] = force          # make sure the value is there, several times
    return x


def _q(dtype, q):
    return (None, None) if dtype == DT_FP32 else ([f32(q[0])], [int(q[1])])


def shuffle_graph(dtype, dims, group, seed=5, in_q=None, out_q=None, force=None):
    """data -> ShuffleChannel -> output.  The reference copies bytes whatever the two tensors' parameters are"""
    in_q = in_q or ((0.05, 0) if dtype == DT_INT8 else (0.05, 77))
    g = Graph(name="shuffle_case")
    x = g.add_input("data", list(dims), dtype, *_q(dtype, in_q))
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, *_q(dtype, out_q or in_q))
    g.output_nodes = [g.add_node("shuffle", "ShuffleChannel", [x], [y], group=group)]
    return g, (_bytes(seed, dtype, dims, force) if dtype != DT_FP32 else np.random.default_rng(seed).normal(0, 1, size=dims).astype(np.float32))


def split_graph(dtype, dims, sizes, seed=5, in_q=None, out_qs=None, cat_q=None, force=None, **kw):
    """data -> Split -> Concat(outputs in reverse order) -> output.  out_qs: per output, None: the input's; cat_q: the Concat's, None: that
    of the Split's LAST output (the Concat's first input)"""
    in_q = in_q or ((0.05, 0) if dtype == DT_INT8 else (0.05, 77))
    out_qs = out_qs or [in_q] * len(sizes)
    g = Graph(name="split_case")
    x = g.add_input("data", list(dims), dtype, *_q(dtype, in_q))
    outs = [g.add_tensor("split_%d" % i, [dims[0], s] + list(dims[2:]), dtype, tm2.TT_VAR, None, *_q(dtype, out_qs[i])) for i, s in enumerate(sizes)]
    g.add_node("split", "Split", [x], outs, axis=kw.pop("axis", 1), split_sizes=list(sizes), **kw)
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, *_q(dtype, cat_q or out_qs[-1]))
    g.output_nodes = [g.add_node("cat", "Concat", outs[::-1], [y], axis=1)]
    return g, (_bytes(seed, dtype, dims, force) if dtype != DT_FP32 else np.random.default_rng(seed).normal(0, 1, size=dims).astype(np.float32))


def split_cat_shuffle_graph(dtype=DT_INT8, dims=(1, 12, 3, 5), sizes=(5, 7), group=3, force=-128):
    """data -> Split -> Concat(outputs in reverse order) -> ShuffleChannel.  The input holds -128, which Split and ShuffleChannel hand on
    and the reference's Concat of several inputs turns into 127 even between equal scales (concat_kernel_ref_int8.c:83-84)"""
    g, x = split_graph(dtype, dims, list(sizes), force=force)
    cat = g.tensors[g.nodes[g.output_nodes[0]].outputs[0]]
    y = g.add_tensor("shuffled", list(dims), dtype, tm2.TT_VAR, None, cat.scales, cat.zero_points)
    g.output_nodes = [g.add_node("shuffle", "ShuffleChannel", [g.nodes[g.output_nodes[0]].outputs[0]], [y], group=group)]
    return g, x


def split_view_graph(dims=(1, 8, 6, 6)):
    """int8 conv (-> 32) -> Split [16, 16]; a 1x1 convolution reads output 0, a 3x3 convolution output 1 (both at the Concat's
    quantisation) -> Concat -> conv1x1: both outputs are channel slices of the first convolution's pixels as they lie"""
    c = Unit(51, DT_INT8, dims)
    c.conv(32, 1)
    a, b = c.split([16, 16])
    ya = c.conv(16, 1, src=a)
    yb = c.conv(16, 3, 1, src=b)
    c.requant(yb, c.quant(ya))
    c.concat([ya, yb], c.quant(ya))
    c.conv(12, 1)
    return c.done()


def shuffle_padding_graph(dtype=DT_INT8, dims=(2, 8, 5, 3)):
    """conv (8 -> 6) -> ShuffleChannel(2) -> conv3x3 pad 1 (6 -> 7): the int8 6-channel tensors have 10 padding lanes per pixel on the
    device and the second convolution's K loop reads them"""
    c = Unit(52, dtype, dims)
    c.conv(6, 1); c.shuffle(2); c.conv(7, 3, 1)
    return c.done()


def basic_unit_graph(dtype, half, dims=(1, 8, 5, 5), seed=53):
    """conv (-> 2 * half) -> the basic unit -> conv1x1"""
    c = Unit(seed, dtype, dims)
    c.conv(2 * half, 1); c.basic_unit(half); c.conv(8, 1)
    return c.done()


def down_unit_graph(dtype=DT_INT8, half=10, dims=(1, 8, 5, 5)):
    c = Unit(54, dtype, dims)
    c.conv(12, 1); c.down_unit(half); c.conv(8, 1)
    return c.done()


def two_units_graph(dims=(1, 3, 32, 32)):
    """int8 stem (conv3x3 + 2x2 max-pool) -> two basic units of half 8 back to back -> global pool -> FC"""
    c = Unit(55, DT_INT8, dims)
    c.conv(16, 3, 1); c.maxpool()
    c.basic_unit(8); c.basic_unit(8)
    c.pool(16, 1)
    c.fc(10)
    return c.done()


def caffe_split_graph(dims=(1, 8, 6, 6)):
    """int8 conv -> is_caffe Split (two full copies) -> conv on each -> Concat: the node the device does not run"""
    c = Unit(56, DT_INT8, dims)
    c.conv(16, 1)
    x = c.cur
    n, ch, h, w = c.dims(x)
    outs = [c._var("copy_%d" % i, [n, ch, h, w], c.quant(x)) for i in range(2)]
    c.g.add_node("split_caffe", "Split", [x], outs, axis=1, is_caffe=1, is_onnx=0)
    ya = c.conv(16, 1, src=outs[0])
    yb = c.conv(16, 1, src=outs[1])
    c.requant(yb, c.quant(ya))
    c.concat([ya, yb], c.quant(ya))
    return c.done()


UNITS = {          # id -> builder(dtype): the unit cases both int8 forms (fused, TAMD_PIN=cat_shuffle=0) run
    "unit_half6": lambda d: basic_unit_graph(d, 6),
    "unit_half16": lambda d: basic_unit_graph(d, 16),
    "unit_half58_b2": lambda d: basic_unit_graph(d, 58, (2, 8, 4, 4)),
    "down_half10": lambda d: down_unit_graph(d, 10),
    "two_units": lambda d: two_units_graph(),
    "split_cat_shuffle_minus128": lambda d: split_cat_shuffle_graph(d),
}


def gpu_cases():
    """{id: (dtype, builder)}: every case the GPU tests run; a builder returns (graph, input)"""
    I8, U8 = DT_INT8, DT_UINT8
    cases = {
        # int8 ShuffleChannel
        "i8_shuffle_one_vector_minus128": (I8, lambda: shuffle_graph(I8, (1, 12, 3, 5), 3, out_q=(0.031, 0), force=-128)),
        "i8_shuffle_cross_vector_batch2": (I8, lambda: shuffle_graph(I8, (2, 20, 3, 2), 2)),
        "i8_shuffle_stage2_width": (I8, lambda: shuffle_graph(I8, (1, 116, 4, 4), 2)),
        "i8_shuffle_ragged_blocks": (I8, lambda: shuffle_graph(I8, (1, 24, 33, 31), 4)),
        "i8_shuffle_group1": (I8, lambda: shuffle_graph(I8, (1, 8, 3, 3), 1)),
        "i8_shuffle_group8": (I8, lambda: shuffle_graph(I8, (1, 8, 3, 3), 8)),
        # int8 Split
        "i8_split_unaligned": (I8, lambda: split_graph(I8, (1, 12, 3, 5), [5, 7])),
        "i8_split_one_aligned_batch2": (I8, lambda: split_graph(I8, (2, 32, 3, 2), [16, 8, 8])),
        "i8_split_views": (I8, split_view_graph),
        "i8_split_scale_differs_minus128": (I8, lambda: split_graph(I8, (1, 12, 3, 5), [5, 7], out_qs=[(0.031, 0), (0.031, 0)], force=-128)),
        # int8 graphs
        "i8_shuffle_padding": (I8, lambda: shuffle_padding_graph(I8)),
        # uint8
        "u8_shuffle_odd_planes": (U8, lambda: shuffle_graph(U8, (1, 3, 5, 7), 3)),
        "u8_shuffle_batch2": (U8, lambda: shuffle_graph(U8, (2, 12, 3, 5), 3)),
        "u8_split_requant_and_identity": (U8, lambda: split_graph(U8, (1, 12, 3, 5), [5, 7], in_q=(0.05, 77), out_qs=[(0.031, 12), (0.05, 77)], cat_q=(0.05, 77))),
        "u8_unit_half6": (U8, lambda: basic_unit_graph(U8, 6)),
    }
    for k, b in UNITS.items():
        cases["i8_" + k] = (I8, lambda b=b: b(I8))
    return cases


def reference_outputs(ref, g, x, dtype):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


def golden():
    return np.load(GOLDEN)


def in_reference_shape(o, shape):
    """a device output under the reference's shape where the two differ in trailing 1s alone: the reference's FC keeps (n, c, 1, 1) behind a
    4-D input, the library infers (n, c) -- the same bytes in the same order"""
    shape = tuple(shape)
    return o.reshape(shape) if o.shape != shape and shape[:o.ndim] == o.shape and all(d == 1 for d in shape[o.ndim:]) else o


def golden_entry(case, outs):
    """the arrays, or for the DIGEST_ONLY cases their shapes and SHA-256"""
    e = {case + "__n": np.int32(len(outs))}
    for i, o in enumerate(outs):
        if case in DIGEST_ONLY:
            e["%s__shape%d" % (case, i)], e["%s__sha%d" % (case, i)] = np.array(o.shape, np.int32), digest(o)
        else:
            e["%s__out%d" % (case, i)] = o
    return e


class _Param:
    @staticmethod
    def split(axis, sizes, num=None):
        p = capi.SplitParam()
        p.axis, p.num = axis, len(sizes) if num is None else num
        for i, s in enumerate(sizes[:capi.SPLIT_MAX]):
            p.sizes[i] = s
        return p


def _desc(dtype, dims, ttype=1, quant=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == DT_FP32 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def ask_split(dtype, in_dims, sizes, axis=1, num=None, out_dims=None, const_input=False, out_quant=None):
    """tamd_node_supported for a Split node; out_dims None: what the reference infers from the sizes"""
    if out_dims is None:
        out_dims = [[in_dims[0], s] + list(in_dims[2:]) for s in sizes] if len(in_dims) >= 2 else [list(in_dims) for _ in sizes]
    p = _Param.split(axis, sizes, num)
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num, n.param = OP_SPLIT, 1, len(out_dims), C.cast(C.pointer(p), C.c_void_p)
    outs = (lh.TensorDesc * max(1, len(out_dims)))(*[_desc(dtype, d, quant=out_quant) for d in out_dims])
    return capi.lib().tamd_node_supported(C.byref(n), (lh.TensorDesc * 1)(_desc(dtype, in_dims, 2 if const_input else 1)), 1, outs, len(out_dims))


def ask_shuffle(dtype, dims, group, const_input=False, with_param=True):
    p = capi.ShuffleChannelParam(group)
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_SHUFFLECHANNEL, 1, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    return capi.lib().tamd_node_supported(C.byref(n), (lh.TensorDesc * 1)(_desc(dtype, dims, 2 if const_input else 1)), 1, (lh.TensorDesc * 1)(_desc(dtype, dims)), 1)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves).  Shape inference and validation run before tamd_graph_prerun
    touches the device, so this answers without a GPU too"""
    return ih.library_output_shape(capi, tm_bytes)
