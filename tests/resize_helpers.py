"""Builders for the tests of the quantised nearest Resize node (tests/test_resize_cpu.py, tests/test_gpu_resize.py,
tools/make_golden_resize.py): single-node graphs with chosen quantisation parameters and scales, the node reading a Concat's buffer and
writing into one between neighbours, and the up-sampling neck conv -> Resize x2 -> Concat(skip) -> conv the plugin must keep whole.
Every case is tmfile bytes with explicit quantisation parameters: the reference library and the device read the same model.  All of it
is batch 1: the reference defines the operator for nothing else.

A node's parameter is written here as the FILE has it, {scale_x, scale_y, type}: the reference's loader fills scale_h from scale_x and
scale_w from scale_y (tm2_resize.c), so scale_x is the factor of the rows."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_cases.npz")
OP_RESIZE = 36          # TAMD_OP_RESIZE
REF_OP_NAME = "Resize"  # the operator's name in the reference's op_name.h, which the plugin's placement report prints
f32 = lh.f32
equals_golden = ih.equals_golden
IN_Q = {DT_UINT8: (0.05, 77), DT_INT8: (0.05, 0)}
OUT_Q = {DT_UINT8: (0.031, 12), DT_INT8: (0.031, 0)}


def scales(sh, sw=None, type_=0):
    """rows by sh, columns by sw (sh when not given), as a file holds them"""
    return {"scale_x": f32(sh), "scale_y": f32(sh if sw is None else sw), "type": int(type_)}


def out_hw(h, w, p):
    """the output size a test WRITES into its tmfile: (int)(H * scale_h), (int)(W * scale_w), the products in float (resize.c:47-48).  The
    reference and the library infer their own; the tests compare those"""
    return int(np.float32(h) * np.float32(p["scale_x"])), int(np.float32(w) * np.float32(p["scale_y"]))


def numpy_indices(n_in, n_out, scale):
    """resize_ref.c:298 / :301 with scale_y = 1.f / scale_h: min((int)(o * (1.f / scale)), n_in - 1), every step in float"""
    inv = np.float32(1.0) / np.float32(scale)
    return np.array([min(int(np.float32(o) * inv), n_in - 1) for o in range(n_out)], np.int32)


def numpy_resize(x, p, table):
    """the whole operator on a (1, C, H, W) array of raw bytes: index vectors, then the byte map"""
    _, _, h, w = x.shape
    oh, ow = out_hw(h, w, p)
    iy, ix = numpy_indices(h, oh, p["scale_x"]), numpy_indices(w, ow, p["scale_y"])
    return table[x.view(np.uint8)[:, :, iy][:, :, :, ix]].view(x.dtype)


def unary_graph(dtype, dims, in_q, out_q, params, out_dims=None, data_const=False, in_quant=None, out_quant=None):
    """input(dims) -> Resize -> output; in_q / out_q: (scale, zero point), None for fp32.  out_dims None: what the reference infers"""
    g = Graph(name="resize_case")
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    if in_quant is not None:
        g.tensors[x].scales, g.tensors[x].zero_points = [f32(in_q[0])] * in_quant, [int(in_q[1])] * in_quant
    src = x
    if data_const:
        src = g.add_const("table", np.zeros(dims, tm2.NP_OF_DT[dtype]), dtype, *q(in_q))
    if out_dims is None:
        out_dims = list(dims[:2]) + list(out_hw(dims[2], dims[3], params)) if len(dims) == 4 else list(dims)
    y = g.add_tensor("out", list(out_dims), dtype, tm2.TT_VAR, None, *q(out_q))
    if out_quant is not None:
        g.tensors[y].scales, g.tensors[y].zero_points = [f32(out_q[0])] * out_quant, [int(out_q[1])] * out_quant
    g.output_nodes = [g.add_node("resize", "Resize", [src], [y], **params)]
    return g


def single(dtype, dims, params, seed, in_q=None, out_q=None, force=None):
    g = unary_graph(dtype, dims, in_q or IN_Q[dtype], out_q or OUT_Q[dtype], params)
    return g, ih._bytes(seed, dtype, dims, force)


class Neck(ih.Neck):
    """interp_helpers.Neck with the Resize node"""

    def resize(self, params, out_q=None, src=None):
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("resize")
        y = self._var(name, [n, c] + list(out_hw(h, w, params)), self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "Resize", [x], [y], **params)
        self.cur = y
        return y

    def done_with(self, outputs, x=None):
        g, x0 = self.done()
        g.output_nodes = list(outputs)
        return g, x0 if x is None else x


def neck_block(dtype, dims=(1, 16, 6, 6), cmid=16, cskip=16, cout=24, seed=91, k=3):
    """the up-sampling of a YOLOv3 / YOLOv4 neck on data (1, C, 2H, 2W): skip = conv1x1(data); low = conv1x1(maxpool 2/2 (data));
    up = Resize x2 (low) at the skip's quantisation; Concat([up, skip]) -> conv k x k.  `dims` are those of the low map"""
    n, c, h, w = dims
    b = Neck(seed, dtype, (n, c, 2 * h, 2 * w))
    data = b.cur
    skip = b.conv(cskip, 1, src=data)
    q = b.quant(skip)
    b.pool(2, 2, src=data)
    b.conv(cmid, 1)
    up = b.resize(scales(2.0), out_q=q)
    b.concat([up, skip], q)
    b.conv(cout, k, k // 2)
    return b.done()


def i8_source_is_a_concat_view(seed=92, dims=(1, 8, 4, 4)):
    """int8: a (16 ch), b (32 ch) = convolutions of data; Concat([a, b]) -> conv; Resize x2 reads b, which lies at channel 16 of the
    Concat's 48-channel pixels: a channel offset and a pixel stride wider than the source's channels (cs_in 48 > C 32)"""
    k = Neck(seed, DT_INT8, dims)
    data = k.cur
    a = k.conv(16, 1, src=data)
    q = k.quant(a)
    b = k.conv(32, 3, 1, src=data)
    k.requant(b, q)
    k.concat([a, b], q)
    k.conv(8, 1)
    head = k.last
    k.resize(scales(2.0), out_q=(0.07, 0), src=b)
    return k.done_with([k.last, head])


def into_concat(dtype, resize_last, cmid=16, lead=16, tail=16, params=None, low_dims=(1, 8, 4, 4), seed=93):
    """Concat([lead conv, Resize(conv(low)), tail conv]) with every input at the Concat's quantisation, so that the node writes its
    channels IN PLACE between neighbours on both sides.  data is the graph's one input, (1, C, OH, OW); the low map is a max-pool of it
    (k = the factor).  resize_last: the node is planned behind both neighbours, else in front of both -- bytes it wrote outside its own
    channels would stay wrong in the one order, bytes a neighbour wrote into its channels in the other.
    uint8: `lead` planes of OH * OW bytes put the node's planes at byte lead * OH * OW of the Concat's image"""
    params = params or scales(2.0)
    f = int(params["scale_x"])
    assert f == params["scale_x"] == params["scale_y"]
    n, c, h, w = low_dims
    k = Neck(seed, dtype, (n, c, h * f, w * f))
    data = k.cur
    q = (0.04, 0) if dtype == DT_INT8 else (0.04, 100)

    def side(ch):
        t = k.conv(ch, 1, src=data)
        k.requant(t, q)
        return t

    def mid():
        k.pool(f, f, src=data)
        k.conv(cmid, 1)
        return k.resize(params, out_q=q)
    if resize_last:
        a, b = side(lead), side(tail)
        m = mid()
    else:
        m = mid()
        a, b = side(lead), side(tail)
    k.concat([a, m, b], q)
    return k.done()


# the single-node cases: id -> (type, input dims, params, kwargs of single()).  What each is for is in tests/test_gpu_resize.py
SINGLE = {}
for _c in (1, 16, 17, 40):
    SINGLE["i8_c%d" % _c] = (DT_INT8, (1, _c, 3, 5), scales(2.0), {})
I8_SCALES = {"2_2": (2.0, 2.0), "2_3": (2.0, 3.0), "3_1": (3.0, 1.0), "1_1": (1.0, 1.0), "1p5_2p5": (1.5, 2.5), "0p5_0p5": (0.5, 0.5)}
for _k, (_sh, _sw) in I8_SCALES.items():
    SINGLE["i8_scale_" + _k] = (DT_INT8, (1, 24, 6, 10), scales(_sh, _sw), {})
SINGLE["i8_equal_minus128"] = (DT_INT8, (1, 5, 3, 4), scales(2.0), dict(in_q=(0.05, 0), out_q=(0.05, 0), force=-128))
SINGLE["u8_planes_of_60"] = (DT_UINT8, (1, 3, 3, 5), scales(2.0), {})                       # OW 10 < 16: no chunk lies inside a row
SINGLE["u8_rows_of_18"] = (DT_UINT8, (1, 2, 4, 9), scales(2.0), {})                         # chunks inside a row and across a row boundary
SINGLE["u8_rows_of_48"] = (DT_UINT8, (1, 3, 5, 24), scales(2.0), {})                        # aligned rows: the doubling path alone
SINGLE["u8_rows_of_36_h3"] = (DT_UINT8, (1, 2, 3, 18), scales(3.0, 2.0), {})                # sw 2 under sh 3; chunks start at columns 0, 16, 32 (-> 12), ...
SINGLE["u8_sw3"] = (DT_UINT8, (1, 3, 3, 7), scales(2.0, 3.0), {})
SINGLE["u8_scale_1_1"] = (DT_UINT8, (1, 3, 5, 7), scales(1.0), {})
SINGLE["u8_shrink"] = (DT_UINT8, (1, 3, 8, 10), scales(0.5), {})
SINGLE["u8_non_integer"] = (DT_UINT8, (1, 3, 6, 10), scales(1.5, 2.5), {})
SINGLE["u8_identity_x2"] = (DT_UINT8, (1, 3, 5, 24), scales(2.0), dict(in_q=(0.05, 77), out_q=(0.05, 77)))
SINGLE["u8_identity_sw3"] = (DT_UINT8, (1, 3, 3, 7), scales(2.0, 3.0), dict(in_q=(0.05, 77), out_q=(0.05, 77)))


def gpu_cases():
    """{id: (type, builder)}: every case the GPU tests run; a builder returns (graph, input)"""
    cases = {k: (dt, (lambda dt=dt, d=d, p=p, kw=kw: single(dt, d, p, 5, **kw))) for k, (dt, d, p, kw) in SINGLE.items()}
    cases["i8_source_concat_view"] = (DT_INT8, i8_source_is_a_concat_view)
    for last in (False, True):
        tag = "resize_last" if last else "resize_first"
        cases["i8_into_concat_" + tag] = (DT_INT8, lambda last=last: into_concat(DT_INT8, last))
        # uint8: one lead plane of 9 x 9 = 81 bytes puts the node's planes at an ODD byte offset (x3: with x2 every plane is even)
        cases["u8_into_concat_odd_offset_" + tag] = (DT_UINT8, lambda last=last: into_concat(DT_UINT8, last, cmid=2, lead=1, tail=2, params=scales(3.0), low_dims=(1, 4, 3, 3)))
    cases["u8_into_concat_x2"] = (DT_UINT8, lambda: into_concat(DT_UINT8, True, cmid=3, lead=1, tail=2, low_dims=(1, 4, 3, 12)))      # planes of 6 x 24 = 144 bytes
    for dt, tag in ((DT_INT8, "i8"), (DT_UINT8, "u8")):
        cases[tag + "_neck_block"] = (dt, lambda dt=dt: neck_block(dt))
    return cases


def rep_is_legal(case):
    """where TAMD_PIN=resize_form=1 gives the replicate kernel (plan_resize): the host-built index vectors are i / sh and j / sw for whole
    numbers -- every case here but the two non-integer scales and the two shrinks"""
    return not any(s in case for s in ("1p5_2p5", "0p5_0p5", "shrink", "non_integer"))


# what runs when TAMD_PIN=resize_form is not set (csrc/kernels.h: kResizeRepFromBytesU8 / I8; profiles/resize.txt has the measurement):
# the replicate kernels from this many output bytes on, where they are legal; form 0 below
REP_FROM_BYTES = {DT_UINT8: 1638400, DT_INT8: 6553600}


def default_form(dtype, out_dims):
    return 1 if int(np.prod(out_dims)) >= REP_FROM_BYTES[dtype] else 0


def expected_kernel(case, form):
    t = "u8" if case.startswith("u8_") else "i8"
    return "resize_rep_" + t if form == 1 and rep_is_legal(case) else "interp_nearest_" + t


def reference_outputs(ref, g, x, dtype):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


def golden():
    return np.load(GOLDEN)


def golden_entry(case, x, outs):
    """a case's seeded input and the reference's outputs"""
    e = {case + "__n": np.int32(len(outs)), case + "__in": x}
    for i, o in enumerate(outs):
        e["%s__out%d" % (case, i)] = o
    return e


def _desc(dtype, dims, ttype=1, quant=None, q=None, keep=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == 0 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    if q is not None and d.quant_num == 1:
        s, z = (C.c_float * 1)(q[0]), (C.c_int * 1)(int(q[1]))
        keep.extend([s, z])
        d.scales, d.zero_points = C.cast(s, C.c_void_p), C.cast(z, C.c_void_p)
    return d


def ask_resize(dtype, in_dims, params, out_dims=None, const_input=False, in_quant=None, out_quant=None, with_param=True, inputs=1, in_q=None, out_q=None):
    """tamd_node_supported for a Resize node (dtype: the C ABI's code; params as a file holds them); out_dims None: what the reference
    infers; in_q / out_q: the quantisation VALUES, where the query is to check the table too"""
    p = capi.ResizeParam(params["scale_y"], params["scale_x"], params["type"])          # {scale_w, scale_h, type}
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_RESIZE, inputs, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    if out_dims is None:
        out_dims = list(in_dims[:2]) + list(out_hw(in_dims[2], in_dims[3], params)) if len(in_dims) == 4 else list(in_dims)
    keep = []
    outs = (lh.TensorDesc * 1)(_desc(dtype, out_dims, quant=out_quant, q=out_q, keep=keep))
    ins = (lh.TensorDesc * 2)(_desc(dtype, in_dims, 2 if const_input else 1, quant=in_quant, q=in_q, keep=keep), _desc(dtype, in_dims))
    return capi.lib().tamd_node_supported(C.byref(n), ins, inputs, outs, 1)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves): both are made before the device is touched.  Without a GPU prerun
    fails at the device for a node that runs; with one it succeeds, and the error is then "" -- tamd_last_error keeps the LAST failure of
    the thread, whichever call that was"""
    L = capi.lib()
    h = L.tamd_graph_load_tm2(tm_bytes, len(tm_bytes))
    assert h
    rc = L.tamd_graph_prerun(h, None)
    dims, dt = (C.c_int * 8)(), C.c_int()
    nd = L.tamd_graph_output_desc(h, 0, dims, C.byref(dt), None, None)
    err = L.tamd_last_error().decode() if rc != 0 else ""
    L.tamd_graph_destroy(h)
    return tuple(dims[k] for k in range(nd)), err
