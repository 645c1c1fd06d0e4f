"""Builders for the tests of the uint8 Slice node (tests/test_slice_cpu.py, tests/test_gpu_slice.py, tools/make_golden_slice.py):
single-node graphs with chosen quantisation parameters and geometry, a chain of two Slices, YOLOv5's Focus layer and a YOLOv4-tiny CSP
block.  Every case is tmfile bytes with explicit quantisation parameters: the reference library and the device read the same model.
(tests/slice_helpers.py is about channel slices of the launchers, another matter.)"""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "slice_cases.npz")
OP_SLICE = 26          # TAMD_OP_SLICE
f32 = lh.f32
digest, equals_golden = ih.digest, ih.equals_golden
DIGEST_ONLY = {"blocks_ragged"}               # ~5 KB of random bytes: the golden holds their shape and SHA-256
IN_Q, OUT_Q = (0.05, 77), (0.031, 12)

# (id, (in scale, in zp), (out scale, out zp)) of the byte map: what each set is for is in its id
TABLE_SETS = [
    ("equal", (0.05, 77), (0.05, 77)),
    ("finer_saturates_at_255", (0.05, 77), (0.031, 12)),
    ("coarser", (0.031, 12), (0.05, 77)),
    ("zp0_to_zp255", (0.05, 0), (0.04, 255)),
    ("zp255_to_zp0", (0.04, 255), (0.05, 0)),
    ("ties", (0.5, 3), (1.0, 4)),              # (b - 3) * 0.5 / 1 + 4: every odd difference lands on an exact .5
    ("awkward_ratio", (0.0173, 101), (0.0291, 37)),
]


def out_extent(dim, begin, end, step):
    """what slice.c:116-156 infers along the axis: end clipped to the dimension, end <= 0 counted from the back, (extent - 1) / step + 1
    for a step above 1 (C division: towards zero), an extent of 0 turned into the dimension"""
    end = min(end, dim)
    e = end - begin if end > 0 else dim + end - begin
    if step > 1:
        e = int((e - 1) / step) + 1
    return dim if e == 0 else e


def numpy_slice(x, axis, begin, end, step):
    """the bytes an onnx Slice picks (before any requantisation)"""
    dim = x.shape[axis]
    end = min(end, dim)
    stop = end if end > 0 else dim + end
    idx = [slice(None)] * x.ndim
    idx[axis] = slice(begin, stop, max(step, 1))
    return x[tuple(idx)]


class Block(ih.Neck):
    """interp_helpers.Neck with Slice and the leaky ReLU of the darknet family"""

    def slice(self, axis, begin, end, step=1, out_q=None, src=None, **kw):
        x = self.cur if src is None else src
        d = self.dims(x)
        ax = axis + len(d) if axis < 0 else axis
        od = list(d)
        od[ax] = out_extent(d[ax], begin, end, step)
        name = self._name("slice")
        y = self._var(name, od, self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "Slice", [x], [y], axis=axis, begin=begin, end=end, step=step, **kw)
        self.cur = y
        return y

    def leaky(self, src=None):
        x = self.cur if src is None else src
        name = self._name("leaky")
        y = self._var(name, self.dims(x), self.quant(x))
        self.last = self.g.add_node(name, "ReLU", [x], [y], negative_slope=f32(0.1))
        self.cur = y
        return y

    def conv_leaky(self, cout, k, src=None):
        self.conv(cout, k, k // 2, src=src)
        return self.leaky()


def slice_graph(dims, axis, begin, end, step=1, in_q=IN_Q, out_q=OUT_Q, seed=5, dtype=DT_UINT8, out_dims=None, outputs=1, **kw):
    """data -> Slice -> output(s); out_dims None: what the reference infers.  kw: iscaffe / ismxnet / isonnx and the three vectors"""
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    g = Graph(name="slice_case")
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    if out_dims is None:
        ax = axis + len(dims) if axis < 0 else axis
        out_dims = list(dims)
        out_dims[ax] = out_extent(dims[ax], begin, end, step)
    ys = [g.add_tensor("out%d" % i if i else "out", list(out_dims), dtype, tm2.TT_VAR, None, *q(out_q)) for i in range(outputs)]
    g.output_nodes = [g.add_node("slice", "Slice", [x], ys, axis=axis, begin=begin, end=end, step=step, **kw)]
    if dtype == DT_FP32:
        return g, np.random.default_rng(seed).normal(0, 1, size=dims).astype(np.float32)
    return g, lh.random_bytes(seed, dtype, dims)


def chain_graph(dims=(1, 3, 8, 12), qs=((0.05, 77), (0.06, 90), (0.043, 140))):
    """data -> Slice(axis 2, begin 1, step 2) -> Slice(axis 3, begin 0, step 2): x[:, :, 1::2, ::2], different parameters on all three tensors"""
    c = Block(61, DT_UINT8, dims, in_q=qs[0])
    c.slice(2, 1, dims[2], 2, out_q=qs[1])
    c.slice(3, 0, dims[3], 2, out_q=qs[2])
    return c.done()


def focus_graph(dims=(1, 3, 12, 20), cout=8, seed=62):
    """YOLOv5's Focus: x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2] -- four chains of Slice(axis 2, step 2) ->
    Slice(axis 3, step 2) -> Concat -> conv3x3.  Every Slice output carries the Concat's quantisation, which is not the input's"""
    c = Block(seed, DT_UINT8, dims)
    data = c.cur
    q = (c.scale(data) * 1.3, 101)
    parts = []
    for hb, wb in ((0, 0), (1, 0), (0, 1), (1, 1)):
        c.slice(2, hb, dims[2], 2, out_q=q, src=data)
        parts.append(c.slice(3, wb, dims[3], 2, out_q=q))
    c.concat(parts, q)
    c.conv(cout, 3, 1)
    return c.done()


def csp_graph(dims=(1, 8, 8, 8), ch=8, seed=63):
    """a YOLOv4-tiny CSP block: conv3x3 -> leaky -> Slice (the second half of the channels: darknet's route groups=2 group_id=1) -> conv ->
    leaky -> conv -> leaky -> Concat(both) -> conv1x1 -> leaky -> Concat(the first conv's output, that) -> 2x2 max-pool"""
    c = Block(seed, DT_UINT8, dims)
    x0 = c.conv_leaky(ch, 3)
    c.slice(1, ch // 2, ch, 1)
    x2 = c.conv_leaky(ch // 2, 3)
    x3 = c.conv_leaky(ch // 2, 3)
    c.concat([x3, x2])
    x4 = c.conv_leaky(ch, 1)
    c.concat([x0, x4])
    c.maxpool()
    return c.done()


def gpu_cases():
    """{id: builder}: every uint8 case the GPU tests run; a builder returns (graph, input).  What each is for is in tests/test_gpu_slice.py"""
    S = slice_graph
    return {
        # channel and batch axes
        "chan_requant": lambda: S((1, 12, 3, 5), 1, 5, 12),
        "chan_batch2_identity": lambda: S((2, 8, 3, 5), 1, 4, 8, out_q=IN_Q),
        "full_range_raw_copy": lambda: S((1, 6, 3, 5), 1, 0, 6),
        "full_range_end_clipped": lambda: S((1, 6, 3, 5), 1, 0, 100),
        "end_negative": lambda: S((1, 8, 3, 5), 1, 1, -2),
        "end_zero": lambda: S((1, 8, 3, 5), 1, 3, 0),
        "batch_axis": lambda: S((3, 4, 3, 5), 0, 1, 3),
        # H and W axes, step 1
        "h_range": lambda: S((1, 3, 7, 5), 2, 2, 6),
        "w_range": lambda: S((1, 3, 4, 37), 3, 3, 36),
        # strided
        "w_step2_even": lambda: S((1, 3, 4, 70), 3, 0, 70, 2),
        "w_step2_odd": lambda: S((1, 3, 4, 70), 3, 1, 70, 2),
        "w_step2_odd_width": lambda: S((1, 3, 4, 71), 3, 1, 71, 2),
        "h_step2": lambda: S((1, 3, 9, 18), 2, 1, 9, 2),
        "c_step3": lambda: S((1, 10, 3, 5), 1, 1, 10, 3),
        "w_step3": lambda: S((1, 2, 3, 50), 3, 0, 50, 3),
        "blocks_ragged": lambda: S((1, 4, 40, 66), 3, 0, 66, 2),
        # two in a row, and the real subgraphs
        "chain": chain_graph,
        "focus": focus_graph,
        "csp": csp_graph,
    }


# the single-node cases: id -> (axis, begin, end, step) as written above, for the tests that restate the pick in numpy
SINGLE = {"chan_requant": (1, 5, 12, 1), "chan_batch2_identity": (1, 4, 8, 1), "full_range_raw_copy": (1, 0, 6, 1), "full_range_end_clipped": (1, 0, 100, 1),
          "end_negative": (1, 1, -2, 1), "end_zero": (1, 3, 0, 1), "batch_axis": (0, 1, 3, 1), "h_range": (2, 2, 6, 1), "w_range": (3, 3, 36, 1),
          "w_step2_even": (3, 0, 70, 2), "w_step2_odd": (3, 1, 70, 2), "w_step2_odd_width": (3, 1, 71, 2), "h_step2": (2, 1, 9, 2), "c_step3": (1, 1, 10, 3),
          "w_step3": (3, 0, 50, 3), "blocks_ragged": (3, 0, 66, 2)}


def reference_outputs(ref, g, x, dtype=DT_UINT8):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


def table_case(in_q, out_q):
    """bytes 0 .. 255 as a (1, 2, 16, 16) tensor through Slice(axis 1, [1, 2)): channel 1 holds byte values 0 .. 255 in order"""
    g, _ = slice_graph((1, 2, 16, 16), 1, 1, 2, in_q=in_q, out_q=out_q)
    x = np.concatenate([np.arange(255, -1, -1, dtype=np.uint8), np.arange(256, dtype=np.uint8)]).reshape(1, 2, 16, 16)
    return g, x


def golden():
    return np.load(GOLDEN)


def golden_entry(case, outs):
    """the arrays, or for the DIGEST_ONLY cases their shapes and SHA-256"""
    e = {case + "__n": np.int32(len(outs))}
    for i, o in enumerate(outs):
        if case in DIGEST_ONLY:
            e["%s__shape%d" % (case, i)], e["%s__sha%d" % (case, i)] = np.array(o.shape, np.int32), digest(o)
        else:
            e["%s__out%d" % (case, i)] = o
    return e


def _desc(dtype, dims, ttype=1, quant=None, q=None, keep=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == DT_FP32 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    if q is not None and d.quant_num >= 1:
        s, z = (C.c_float * d.quant_num)(*[f32(q[0])] * d.quant_num), (C.c_int * d.quant_num)(*[int(q[1])] * d.quant_num)
        keep += [s, z]
        d.scales, d.zero_points = C.cast(s, C.c_void_p), C.cast(z, C.c_void_p)
    return d


def ask_slice(dtype, in_dims, axis, begin, end, step=1, out_dims=None, outputs=1, const_input=False, in_quant=None, out_quant=None, in_q=IN_Q, out_q=OUT_Q,
              with_param=True, iscaffe=0, ismxnet=0, isonnx=1, slice_point_num=0, begin_num=0, size_num=0):
    """tamd_node_supported for a Slice node; out_dims None: what the reference infers"""
    if out_dims is None:
        ax = axis + len(in_dims) if axis < 0 else axis
        out_dims = list(in_dims)
        if 0 <= ax < len(in_dims):
            out_dims[ax] = out_extent(in_dims[ax], begin, end, step)
    keep = []
    p = capi.SliceParam(axis, begin, end, step, iscaffe, ismxnet, isonnx, slice_point_num, begin_num, size_num)
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_SLICE, 1, outputs
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    outs = (lh.TensorDesc * outputs)(*[_desc(dtype, out_dims, quant=out_quant, q=out_q, keep=keep) for _ in range(outputs)])
    ins = (lh.TensorDesc * 1)(_desc(dtype, in_dims, 2 if const_input else 1, quant=in_quant, q=in_q, keep=keep))
    return capi.lib().tamd_node_supported(C.byref(n), ins, 1, outs, outputs)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves).  Shape inference and validation run before tamd_graph_prerun
    touches the device, so this answers without a GPU too"""
    return ih.library_output_shape(capi, tm_bytes)
