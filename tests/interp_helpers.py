"""Builders for the tests of the quantised nearest Interp node (tests/test_interp_cpu.py, tests/test_gpu_interp.py, tools/make_golden_interp.py):
single-node graphs with chosen quantisation parameters and geometry, and the graphs around the node that the device kernels can get wrong
-- padding lanes in front of a convolution, concat in place and by copy, the FPN / PAN neck of the YOLOv5 family.  Every case is tmfile
bytes with explicit quantisation parameters: the reference library and the device read the same model."""
import ctypes as C
import hashlib
import os

import numpy as np

import lut_helpers as lh
from tengine_amd import tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "interp_nearest_cases.npz")
OP_INTERP = 20          # TAMD_OP_INTERP
f32 = lh.f32


def by_scale(hs, ws=None, resize_type=1):
    """both scales set: the sizes are not read (interp.c:51-55)"""
    return {"resize_type": resize_type, "width_scale": f32(hs if ws is None else ws), "height_scale": f32(hs), "output_width": 0, "output_height": 0}


def by_size(oh, ow, resize_type=1):
    """scales 0 in the file: the sizes decide (interp.c:56-60)"""
    return {"resize_type": resize_type, "width_scale": 0.0, "height_scale": 0.0, "output_width": int(ow), "output_height": int(oh)}


def out_hw(h, w, p):
    """the output size a test WRITES into its tmfile (the reference and the library infer their own; the tests compare those)"""
    if p["height_scale"] != 0 and p["width_scale"] != 0:
        return int(np.float32(h) * np.float32(p["height_scale"])), int(np.float32(w) * np.float32(p["width_scale"]))
    return p["output_height"], p["output_width"]


def unary_graph(dtype, dims, in_q, out_q, params):
    """input(dims) -> Interp -> output; in_q / out_q: (scale, zero point), None for fp32"""
    g = Graph(name="interp_case")
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    oh, ow = out_hw(dims[2], dims[3], params) if len(dims) == 4 else (1, 1)
    y = g.add_tensor("out", list(dims[:2]) + [oh, ow] if len(dims) == 4 else list(dims), dtype, tm2.TT_VAR, None, *q(out_q))
    g.output_nodes = [g.add_node("interp", "Interp", [x], [y], **params)]
    return g


class Neck(lh.Chain):
    """lut_helpers.Chain with the nodes of a detector's neck: Interp, channel Concat, pooling with any window"""

    def quant(self, t):
        x = self.g.tensors[t]
        return None if self.dtype == DT_FP32 else (x.scales[0], x.zero_points[0])

    def requant(self, t, q):
        """give tensor t the quantisation q (a concat input must carry the concat's to be written in place)"""
        if self.dtype != DT_FP32:
            self.g.tensors[t].scales, self.g.tensors[t].zero_points = [f32(q[0])], [int(q[1])]

    def interp(self, params, out_q=None, src=None):
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("interp")
        y = self._var(name, [n, c] + list(out_hw(h, w, params)), self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "Interp", [x], [y], **params)
        self.cur = y
        return y

    def concat(self, xs, q=None):
        d = self.dims(xs[0])
        name = self._name("cat")
        y = self._var(name, [d[0], sum(self.dims(t)[1] for t in xs)] + d[2:], self.quant(xs[0]) if q is None else q)
        self.last = self.g.add_node(name, "Concat", list(xs), [y], axis=1)
        self.cur = y
        return y

    def pool(self, k, s, pad=0, src=None):
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("pool")
        y = self._var(name, [n, c, (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1], self.quant(x))
        self.last = self.g.add_node(name, "Pooling", [x], [y], alg=0, kernel_h=k, kernel_w=k, stride_h=s, stride_w=s, **{"global": 0},
                                    caffe_flavor=0, pad_h0=pad, pad_w0=pad, pad_h1=pad, pad_w1=pad)
        self.cur = y
        return y


def _in_q(dtype):
    return (0.05, 0) if dtype == DT_INT8 else (0.05, 77)


def _out_q(dtype):
    return (0.031, 0) if dtype == DT_INT8 else (0.031, 12)


def _bytes(seed, dtype, dims, force=None):
    x = lh.random_bytes(seed, dtype, dims)
    if force is not None:
        x.reshape(-1)[:: max(1, x.size // 7)] = force          # make sure the value is there, several times
    return x


def single(dtype, dims, params, seed, in_q=None, out_q=None, force=None):
    g = unary_graph(dtype, dims, in_q or _in_q(dtype), out_q or _out_q(dtype), params)
    return g, _bytes(seed, dtype, dims, force)


def padding_graph(dtype, dims=(2, 8, 5, 3)):
    """conv1x1 (8 -> 5) -> Interp x2 -> conv3x3 pad 1 (5 -> 7): the int8 5-channel tensors have 11 padding lanes per pixel on the device
    and the second convolution's K loop reads them: whatever the Interp kernel leaves there is in the second convolution's sums"""
    c = Neck(41, dtype, dims)
    c.conv(5, 1)
    c.interp(by_scale(2.0), out_q=(c.scale() * 0.7, 0 if dtype == DT_INT8 else 12))
    c.conv(7, 3, 1)
    return c.done()


def concat_graph(dtype, cin, lead=0, k=2):
    """data (1, 8, S, S), S = 8 (k 2) or 9 (k 3) -> conv (32 ch) = skip; data -> pool k / k -> conv (cin ch) -> Interp xk -> Concat([lead conv,] interp, skip) with
    every input at the concat's quantisation.  cin 16 and no lead: both inputs of the int8 concat are written in place.  cin 8: neither
    int8 slice is a multiple of 16 channels, the concat copies.  lead > 0 (uint8): a `lead`-channel convolution in front makes the Interp's
    planes start at byte lead * OH * OW of the concat's image"""
    side = {2: 8, 3: 9}[k]
    c = Neck(42, dtype, (1, 8, side, side))
    data = c.cur
    skip = c.conv(32, 1, src=data)
    q = c.quant(skip)
    ins = []
    if lead:
        ins.append(c.conv(lead, 1, src=data))
        c.requant(ins[-1], q)
    c.pool(k, k, src=data)
    c.conv(cin, 1)
    ins.append(c.interp(by_scale(float(k)), out_q=q))
    ins.append(skip)
    c.concat(ins, q)
    return c.done()


def neck_graph(dtype, dims=(1, 16, 8, 8)):
    """the neck of YOLOv5 / YOLOX: a = conv(data) is the skip; low = conv(pool 2 / 2 (a)); an SPP over it (max-pool 5 / 9 / 13, stride 1,
    pad 2 / 4 / 6 -> Concat) -> conv -> SiLU (Sigmoid, Eltwise PROD) -> Interp x2 -> Concat(skip) -> conv3x3"""
    c = Neck(43, dtype, dims)
    a = c.conv(16, 1)
    c.pool(2, 2)
    low = c.conv(16, 1)
    spp = c.concat([low] + [c.pool(k, 1, k // 2, src=low) for k in (5, 9, 13)])
    b = c.conv(16, 1, src=spp)
    s = c.act("Sigmoid")
    c.prod(b, s)
    up = c.interp(by_scale(2.0), out_q=c.quant(a))
    c.concat([up, a])
    c.conv(24, 3, 1)
    return c.done()


def bilinear_graph(dims=(1, 8, 6, 6)):
    """int8 conv -> bilinear Interp x2 -> conv: the node the device does not run"""
    c = Neck(44, DT_INT8, dims)
    c.conv(16, 3, 1); c.interp(by_scale(2.0, resize_type=2)); c.conv(12, 1)
    return c.done()


# the geometry rows both precisions run: id -> (dims, params)
GEOMETRY = {
    "batch_per_axis": ((2, 17, 5, 3), by_scale(2.0, 3.0)),          # two vectors per int8 pixel, image stride, h x2, w x3
    "non_integer": ((1, 16, 7, 4), by_scale(1.5)),                  # -> 10 x 6
    "down": ((1, 16, 8, 8), by_scale(0.5)),
    "sizes_only": ((1, 8, 5, 5), by_size(7, 7)),
    "ragged_blocks": ((1, 24, 33, 31), by_scale(2.0)),              # several blocks, the last one partial
}
DIGEST_ONLY = {"ragged_blocks"}                                     # ~200 KB of random bytes: the golden holds their shape and SHA-256


def gpu_cases():
    """{id: (dtype, builder)}: every case the GPU tests run; a builder returns (graph, input)"""
    cases = {}
    for dtype, tag in ((DT_INT8, "i8"), (DT_UINT8, "u8")):
        cases[tag + "_padding"] = (dtype, lambda d=dtype: padding_graph(d))
        for k, (dims, p) in GEOMETRY.items():
            cases["%s_%s" % (tag, k)] = (dtype, lambda d=dtype, dims=dims, p=p: single(d, dims, p, 5))
        cases[tag + "_neck"] = (dtype, lambda d=dtype: neck_graph(d))
    cases["i8_one_vector_minus128"] = (DT_INT8, lambda: single(DT_INT8, (1, 5, 3, 4), by_scale(2.0), 6, force=-128))
    cases["i8_concat_in_place"] = (DT_INT8, lambda: concat_graph(DT_INT8, 16))
    cases["i8_concat_fallback"] = (DT_INT8, lambda: concat_graph(DT_INT8, 8))
    cases["u8_odd_planes"] = (DT_UINT8, lambda: single(DT_UINT8, (1, 3, 5, 7), by_scale(2.0), 6))       # zero points 77 in, 12 out
    cases["u8_identity"] = (DT_UINT8, lambda: single(DT_UINT8, (1, 3, 5, 7), by_scale(1.5, 3.0), 7, in_q=(0.05, 77), out_q=(0.05, 77)))
    cases["u8_concat_in_place_odd_start"] = (DT_UINT8, lambda: concat_graph(DT_UINT8, 5, lead=3, k=3))
    return cases


def reference_outputs(ref, g, x, dtype):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


def golden():
    return np.load(GOLDEN)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def golden_entry(case, outs):
    """what the golden stores for a case's reference outputs: the arrays, or for the DIGEST_ONLY cases their shapes and SHA-256"""
    e = {case + "__n": np.int32(len(outs))}
    for i, o in enumerate(outs):
        if case.split("_", 1)[1] in DIGEST_ONLY:
            e["%s__shape%d" % (case, i)], e["%s__sha%d" % (case, i)] = np.array(o.shape, np.int32), digest(o)
        else:
            e["%s__out%d" % (case, i)] = o
    return e


def equals_golden(z, case, outs):
    """do these outputs equal what the golden holds for the case?  (shape, type and every byte; by digest for the DIGEST_ONLY cases)"""
    if len(outs) != int(z[case + "__n"]):
        return False
    for i, o in enumerate(outs):
        key = "%s__out%d" % (case, i)
        if key in z.files:
            if not (z[key].shape == o.shape and z[key].dtype == o.dtype and np.array_equal(z[key], o)):
                return False
        elif not (tuple(z["%s__shape%d" % (case, i)]) == o.shape and np.array_equal(z["%s__sha%d" % (case, i)], digest(o))):
            return False
    return True


def library_output_shape(capi, tm_bytes):
    """the shape the library infers for output 0.  Shape inference and validation run before tamd_graph_prerun touches the device, so
    this answers without a GPU too (prerun then fails at the device; with one it succeeds)"""
    L = capi.lib()
    h = L.tamd_graph_load_tm2(tm_bytes, len(tm_bytes))
    assert h
    L.tamd_graph_prerun(h, None)
    dims, dt = (C.c_int * 8)(), C.c_int()
    nd = L.tamd_graph_output_desc(h, 0, dims, C.byref(dt), None, None)
    err = L.tamd_last_error().decode()
    L.tamd_graph_destroy(h)
    return tuple(dims[k] for k in range(nd)), err


class InterpParam(C.Structure):         # tamd_interp_param
    _fields_ = [("resize_type", C.c_int), ("width_scale", C.c_float), ("height_scale", C.c_float), ("output_width", C.c_int), ("output_height", C.c_int)]


def ask_node(capi, dtype, in_dims, params, out_dims=None, const_input=False):
    """tamd_node_supported for an Interp node; out_dims None: what the reference would have inferred (out_hw)"""
    if out_dims is None:
        out_dims = list(in_dims[:2]) + list(out_hw(in_dims[2], in_dims[3], params)) if len(in_dims) == 4 else list(in_dims)

    def t(dims, ttype):
        d = lh.TensorDesc()
        d.dtype, d.ttype, d.dim_num, d.quant_num = dtype, ttype, len(dims), 0 if dtype == DT_FP32 else 1
        for i, v in enumerate(dims):
            d.dims[i] = v
        return d
    p = InterpParam(params["resize_type"], params["width_scale"], params["height_scale"], params["output_width"], params["output_height"])
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num, n.param = OP_INTERP, 1, 1, C.cast(C.pointer(p), C.c_void_p)
    return capi.lib().tamd_node_supported(C.byref(n), (lh.TensorDesc * 1)(t(in_dims, 2 if const_input else 1)), 1, (lh.TensorDesc * 1)(t(out_dims, 1)), 1)
