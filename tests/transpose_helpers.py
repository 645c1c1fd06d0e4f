"""Builders for the tests of the quantised Transpose node (tests/test_transpose_cpu.py, tests/test_gpu_transpose.py): single-node graphs
with chosen quantisation parameters and geometry, the int8 forms that read a convolution-stack buffer where it lies, the Detect head of
the YOLOv5 family, torch's channel shuffle and a Transpose that moves the batch axis.  Every case is tmfile bytes with explicit
quantisation parameters: the reference library and the device read the same model.

    python tests/transpose_helpers.py          writes tests/golden/transpose_cases.npz (needs oracle/_ref/libtengine-lite.so)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import interp_helpers as ih  # noqa: E402
import lut_helpers as lh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "transpose_cases.npz")
OP_TRANSPOSE = 28      # TAMD_OP_TRANSPOSE (27 is reserved)
f32 = lh.f32
digest, equals_golden = ih.digest, ih.equals_golden
DIGEST_ONLY = {"u8_tile_edges_65x67"}          # ~4 KB of random bytes: the golden holds their shape and SHA-256
# uint8: the pair the Slice tests use; it saturates at both ends ((0 - 77) * 0.05 / 0.031 + 12 < 0, (255 - 77) * 0.05 / 0.031 + 12 > 255)
U8_IN, U8_OUT = (0.05, 77), (0.031, 12)
I8_IN, I8_OUT = (0.05, 0), (0.031, 0)

# (id, (in scale, in zp), (out scale, out zp)) of the byte map, per type: what each set is for is in its id
TABLE_SETS = {
    DT_UINT8: [
        ("equal", (0.05, 77), (0.05, 77)),
        ("finer_saturates_at_0_and_255", (0.05, 77), (0.031, 12)),
        ("coarser", (0.031, 12), (0.05, 77)),
        ("zp0_to_zp255", (0.05, 0), (0.04, 255)),
        ("zp255_to_zp0", (0.04, 255), (0.05, 0)),
        ("ties", (0.5, 3), (1.0, 4)),          # (b - 3) * 0.5 / 1 + 4: every odd difference lands on an exact .5
        ("awkward_ratio", (0.0173, 101), (0.0291, 37)),
        ("equal_zp0", (0.02, 0), (0.02, 0)),
    ],
    DT_INT8: [
        ("equal", (0.05, 0), (0.05, 0)),                          # -128 -> -127, everything else itself
        ("finer_saturates_at_pm127", (0.05, 0), (0.031, 0)),      # -128 * 0.05 / 0.031 = -206 -> -127, 127 -> 205 -> 127
        ("coarser", (0.031, 0), (0.05, 0)),
        ("in_zp_nonzero", (0.05, 9), (0.04, 0)),
        ("out_zp_nonzero", (0.05, 0), (0.04, -11)),
        ("both_zp_nonzero_saturates", (0.05, -30), (0.02, 25)),
        ("ties", (0.5, 3), (1.0, 4)),
        ("awkward_ratio", (0.0173, 5), (0.0291, -7)),
    ],
}


def q_of(dtype, q):
    return (None, None) if dtype == DT_FP32 else ([f32(q[0])], [int(q[1])])


def transpose_graph(dtype, dims, order, in_q=None, out_q=None, seed=5, out_dims=None, force=None):
    """data -> Transpose -> output; out_dims None: what the reference infers; order None: a node without its tr_shape vector"""
    in_q = in_q or (I8_IN if dtype == DT_INT8 else U8_IN)
    out_q = out_q or (I8_OUT if dtype == DT_INT8 else U8_OUT)
    g = Graph(name="transpose_case")
    x = g.add_input("data", list(dims), dtype, *q_of(dtype, in_q))
    if out_dims is None:
        out_dims = [dims[o] for o in order]
    y = g.add_tensor("out", list(out_dims), dtype, tm2.TT_VAR, None, *q_of(dtype, out_q))
    g.output_nodes = [g.add_node("transpose", "Transpose", [x], [y], tr_shape=None if order is None else list(order))]
    if dtype == DT_FP32:
        return g, np.random.default_rng(seed).normal(0, 1, size=dims).astype(np.float32)
    data = lh.random_bytes(seed, dtype, dims)
    if force is not None:
        data.reshape(-1)[:: max(1, data.size // 7)] = force
    return g, data


class Block(ih.Neck):
    """interp_helpers.Neck with Reshape (unique names, any rank), Transpose and a Concat along any axis"""

    def reshape(self, dims, src=None):
        x = self.cur if src is None else src
        name = self._name("reshape")
        y = self._var(name, list(dims), self.quant(x))
        self.last = self.g.add_node(name, "Reshape", [x], [y], is_mxnet=0, reverse=0, is_onnx=1, re_shape=list(dims))
        self.cur = y
        return y

    def transpose(self, order, out_q=None, src=None):
        x = self.cur if src is None else src
        d = self.dims(x)
        name = self._name("transpose")
        y = self._var(name, [d[o] for o in order], self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "Transpose", [x], [y], tr_shape=list(order))
        self.cur = y
        return y

    def concat_axis(self, xs, axis, q=None):
        d = self.dims(xs[0])
        d[axis] = sum(self.dims(t)[axis] for t in xs)
        name = self._name("cat")
        y = self._var(name, d, self.quant(xs[0]) if q is None else q)
        self.last = self.g.add_node(name, "Concat", list(xs), [y], axis=axis)
        self.cur = y
        return y

    def done_outputs(self, nodes, seed=1):
        g, x = self.done(seed)
        g.output_nodes = list(nodes)
        return g, x


def _finer(c, dtype, t=None):
    """another quantisation than tensor t's: a finer scale (saturates some values), another zero point in uint8"""
    return (c.scale(t) * 0.7, 0 if dtype == DT_INT8 else 140)


def i8_input_graph(in_q=(0.05, 0), out_q=(0.05, 0), force=-128):
    """int8 graph input (2, 6, 4, 5) -> Transpose (0, 2, 3, 1): the input is a convolution-stack buffer on the device (6 channels in a pixel
    of 16 bytes) and is read where it lies.  The input holds -128, which comes out as -127 even between equal parameters"""
    return transpose_graph(DT_INT8, (2, 6, 4, 5), (0, 2, 3, 1), in_q, out_q, seed=31, force=force)


def i8_view_graph(reshape=(1, 2, 3, 20), order=(0, 2, 1, 3), seed=32):
    """int8 conv1x1 (8 -> 6 channels: 16 bytes per pixel) on (1, 8, 4, 5) -> Reshape -> Transpose.  (1, 2, 3, 20) splits C into 2 x 3 and keeps
    H * W whole: the Transpose reads the convolution's buffer through the Reshape.  (1, 3, 8, 5) mixes C with H: the Reshape copies"""
    c = Block(seed, DT_INT8, (1, 8, 4, 5))
    c.conv(6, 1)
    c.reshape(reshape)
    c.transpose(order, out_q=_finer(c, DT_INT8))
    return c.done()


def i8_concat_view_graph():
    """int8 Concat(conv 16 ch, conv 4 ch) = 20 channels in pixels of 32 bytes -> Reshape (1, 4, 5, 20) -> Transpose (0, 2, 1, 3), and a second
    Transpose (0, 2, 3, 1) that reads the 16-channel convolution of ANOTHER Concat where it lies in that Concat's buffer: a channel slice at
    offset 16 of 32-byte pixels"""
    c = Block(33, DT_INT8, (1, 8, 4, 5))
    data = c.cur
    a = c.conv(16, 1, src=data)
    b = c.conv(4, 1, src=data)
    c.requant(b, c.quant(a))
    c.concat([a, b])
    c.reshape((1, 4, 5, 20))
    c.transpose((0, 2, 1, 3), out_q=_finer(c, DT_INT8))
    t1 = c.last
    p = c.conv(16, 1, src=data)
    s = c.conv(16, 1, src=data)
    c.requant(s, c.quant(p))
    c.concat([p, s])
    c.conv(8, 1)
    o2 = c.last
    c.transpose((0, 2, 3, 1), out_q=_finer(c, DT_INT8, s), src=s)
    return c.done_outputs([t1, o2, c.last])


def i8_dense_chain_graph():
    """int8 conv -> Reshape (1, 2, 3, 20) -> Transpose (0, 2, 1, 3) -> Transpose (0, 1, 3, 2): the second reads a dense tensor"""
    c = Block(34, DT_INT8, (1, 8, 4, 5))
    c.conv(6, 1)
    c.reshape((1, 2, 3, 20))
    c.transpose((0, 2, 1, 3), out_q=_finer(c, DT_INT8))
    c.transpose((0, 1, 3, 2), out_q=(c.scale() * 1.3, 0))
    return c.done()


def detect_graph(dtype, batch=2, anchors=3, values=7, cin=8, side=4, seed=35):
    """the Detect head of the YOLOv5 family at two scales (side x side and half of it): per scale conv1x1 (cin -> anchors * values) ->
    Reshape (N, anchors, values, H, W) -> Transpose (0, 1, 3, 4, 2) -> Sigmoid -> Reshape (N, anchors * H * W, values); Concat (axis 1)"""
    c = Block(seed, dtype, (batch, cin, side, side))
    data = c.cur
    heads = []
    for k in range(2):
        c.cur = data
        src = data if k == 0 else c.maxpool()
        s = side >> k
        c.conv(anchors * values, 1, src=src)
        c.reshape((batch, anchors, values, s, s))
        c.transpose((0, 1, 3, 4, 2), out_q=_finer(c, dtype))
        c.act("Sigmoid")                       # (both heads get the same output quantisation: the Concat's)
        heads.append(c.reshape((batch, anchors * s * s, values)))
    c.concat_axis(heads, 1)
    return c.done()


def shuffle_graph(seed=36):
    """torch's channel shuffle in uint8, batch 2: conv -> Reshape (2, 2, 4, 3, 5) -> Transpose (0, 2, 1, 3, 4) -> Reshape (2, 8, 3, 5) -> conv"""
    c = Block(seed, DT_UINT8, (2, 8, 3, 5))
    c.conv(8, 1)
    c.reshape((2, 2, 4, 3, 5))
    c.transpose((0, 2, 1, 3, 4), out_q=_finer(c, DT_UINT8))
    c.reshape((2, 8, 3, 5))
    c.conv(6, 3, 1)
    return c.done()


def batch_axis_graph(seed=37):
    """uint8 conv (8 -> 4 channels) on (4, 8, 3, 5) -> Transpose (1, 0, 2, 3): every tensor carries 4 as dimension 0 and every other operator
    treats the images independently, so only the Transpose keeps the graph from being compiled as two half-batch graphs"""
    c = Block(seed, DT_UINT8, (4, 8, 3, 5))
    c.conv(4, 1)
    c.transpose((1, 0, 2, 3), out_q=_finer(c, DT_UINT8))
    return c.done()


# the uint8 single-node cases: id -> (dims, order, in_q, out_q); None: U8_IN / U8_OUT.  What each is for is in tests/test_gpu_transpose.py
U8_SINGLE = {
    "u8_2d": ((5, 7), (1, 0), None, None),
    "u8_3d_021": ((2, 5, 7), (0, 2, 1), None, None),
    "u8_3d_201": ((2, 5, 7), (2, 0, 1), None, None),
    "u8_3d_102": ((2, 5, 7), (1, 0, 2), None, None),
    "u8_4d_nhwc": ((1, 6, 5, 7), (0, 2, 3, 1), None, None),
    "u8_4d_reversed": ((2, 3, 4, 5), (3, 2, 1, 0), None, None),
    "u8_4d_inner_swap": ((2, 3, 4, 5), (0, 1, 3, 2), None, None),
    "u8_4d_identity_order": ((2, 3, 4, 5), (0, 1, 2, 3), None, None),
    "u8_5d_shuffle": ((1, 2, 3, 4, 5), (0, 2, 1, 3, 4), None, None),
    "u8_5d_detect": ((2, 3, 11, 3, 5), (0, 1, 3, 4, 2), None, None),
    "u8_6d": ((1, 2, 3, 2, 3, 5), (0, 1, 4, 2, 5, 3), None, None),
    "u8_size1_axes": ((1, 1, 5, 1, 7), (4, 3, 2, 1, 0), None, None),
    "u8_tile_edges_65x67": ((1, 65, 67), (0, 2, 1), None, None),
    "u8_tile_edges_130x3": ((3, 130, 3), (0, 2, 1), None, None),
    "u8_rows_1": ((2, 3, 1), (1, 0, 2), None, None),
    "u8_rows_15": ((2, 3, 15), (1, 0, 2), None, None),
    "u8_rows_16": ((2, 3, 16), (1, 0, 2), None, None),
    "u8_rows_17": ((2, 3, 17), (1, 0, 2), None, None),
    "u8_rows_33": ((2, 3, 33), (1, 0, 2), None, None),
    "u8_equal_params_tile": ((2, 5, 7), (0, 2, 1), (0.05, 77), (0.05, 77)),
    "u8_equal_params_rows": ((2, 3, 33), (1, 0, 2), (0.05, 77), (0.05, 77)),
    "u8_coarser": ((2, 5, 7), (2, 0, 1), (0.031, 12), (0.05, 77)),
}


def gpu_cases():
    """{id: (dtype, builder)}: every case the GPU tests run; a builder returns (graph, input)"""
    cases = {}
    for k, (dims, order, in_q, out_q) in U8_SINGLE.items():
        cases[k] = (DT_UINT8, lambda dims=dims, order=order, in_q=in_q, out_q=out_q: transpose_graph(DT_UINT8, dims, order, in_q, out_q))
    cases["i8_input_nhwc_minus128"] = (DT_INT8, i8_input_graph)
    cases["i8_input_saturates"] = (DT_INT8, lambda: i8_input_graph((0.05, 0), (0.02, 0), force=None))
    cases["i8_view"] = (DT_INT8, i8_view_graph)
    cases["i8_mixed_reshape"] = (DT_INT8, lambda: i8_view_graph((1, 3, 8, 5), (0, 2, 1, 3), 38))
    cases["i8_concat_view"] = (DT_INT8, i8_concat_view_graph)
    cases["i8_dense_chain"] = (DT_INT8, i8_dense_chain_graph)
    cases["i8_detect"] = (DT_INT8, lambda: detect_graph(DT_INT8))
    cases["u8_detect"] = (DT_UINT8, lambda: detect_graph(DT_UINT8))
    cases["u8_shuffle"] = (DT_UINT8, shuffle_graph)
    cases["u8_batch_axis"] = (DT_UINT8, batch_axis_graph)
    return cases


def reference_outputs(ref, g, x, dtype):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


def table_case(dtype, in_q, out_q):
    """the byte values 0 .. 255 (raw bytes, in order) as channel 1 of a (1, 2, 16, 16) tensor through the identity-order Transpose"""
    g, _ = transpose_graph(dtype, (1, 2, 16, 16), (0, 1, 2, 3), in_q, out_q)
    x = np.concatenate([np.arange(255, -1, -1, dtype=np.uint8), np.arange(256, dtype=np.uint8)]).view(lh.NP[dtype]).reshape(1, 2, 16, 16)
    return g, x


def table_of(dtype, in_q, out_q):
    return capi.transpose_table(dtype, f32(in_q[0]), int(in_q[1]), f32(out_q[0]), int(out_q[1]))


def table_key(dtype, name):
    return "table__%s__%s" % ("i8" if dtype == DT_INT8 else "u8", name)


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


def write_golden():
    """tests/golden/transpose_cases.npz: for every GPU case (seeded inputs) the outputs of the real reference library, and under
    table__<type>__<id> the 256 bytes the reference's Transpose makes of the byte values 0 .. 255 for every parameter pair of TABLE_SETS.
    tests/test_transpose_cpu.py::test_golden_is_the_real_reference checks the file against the reference wherever that exists"""
    from oracle import ref_capi as ref
    assert ref.available(), "build the reference library first (oracle/build_ref.py)"
    z = {}
    for case, (dtype, build) in sorted(gpu_cases().items()):
        g, x = build()
        z.update(golden_entry(case, reference_outputs(ref, g, x, dtype)))
    for dtype, sets in TABLE_SETS.items():
        for name, in_q, out_q in sets:
            g, x = table_case(dtype, in_q, out_q)
            z[table_key(dtype, name)] = reference_outputs(ref, g, x, dtype)[0][0, 1].reshape(-1)
    np.savez_compressed(GOLDEN, **z)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(z), "arrays")


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


def ask_transpose(dtype, in_dims, order, out_dims=None, const_input=False, in_quant=None, out_quant=None, in_q=None, out_q=None, with_param=True):
    """tamd_node_supported for a Transpose node; out_dims None: what the reference infers"""
    in_q = in_q or (I8_IN if dtype == DT_INT8 else U8_IN)
    out_q = out_q or (I8_OUT if dtype == DT_INT8 else U8_OUT)
    if out_dims is None:
        out_dims = [in_dims[o] if 0 <= o < len(in_dims) else 1 for o in order]
    keep = []
    p = capi.TransposeParam()
    p.dim_num = len(order)
    for i, o in enumerate(order[:8]):
        p.order[i] = o
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_TRANSPOSE, 1, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    outs = (lh.TensorDesc * 1)(_desc(dtype, out_dims, quant=out_quant, q=out_q, keep=keep))
    ins = (lh.TensorDesc * 1)(_desc(dtype, in_dims, 2 if const_input else 1, quant=in_quant, q=in_q, keep=keep))
    return capi.lib().tamd_node_supported(C.byref(n), ins, 1, outs, 1)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves).  Shape inference and validation run before tamd_graph_prerun
    touches the device, so this answers without a GPU too"""
    return ih.library_output_shape(capi, tm_bytes)


if __name__ == "__main__":
    write_golden()
