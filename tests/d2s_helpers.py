"""Builders for the tests of the quantised DepthToSpace node (tests/test_d2s_cpu.py, tests/test_gpu_d2s.py, tools/make_golden_d2s.py):
single-node graphs in both quantised types, the node writing into and reading out of Concat buffers, and the two sub-pixel-convolution
graphs the plugin must keep whole.  Every case is tmfile bytes with explicit quantisation parameters: the reference library and the
device read the same model.  The expected bytes are numpy_d2s below; tests/golden/d2s_cases.npz pins that statement to the real
reference."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "d2s_cases.npz")
OP_DEPTHTOSPACE = 34    # TAMD_OP_DEPTHTOSPACE
REF_OP_NAME = "Depthtospace"      # the operator's name in the reference's op_name.h, which the plugin's placement report prints
f32 = lh.f32
equals_golden = ih.equals_golden
# the two tensors of a node carry DIFFERENT parameters in every single-node case: the reference copies the bytes regardless
IN_Q = {DT_UINT8: (0.05, 77), DT_INT8: (0.05, 0)}
OUT_Q = {DT_UINT8: (0.031, 12), DT_INT8: (0.031, 0)}


def numpy_d2s(x, r):
    """depthtospace_ref.c, the CRD order: out[b, s, h, w] = in[b, s * r * r + (h % r) * r + (w % r), h / r, w / r]"""
    n, c, h, w = x.shape
    outc = c // (r * r)
    return np.ascontiguousarray(x.reshape(n, outc, r, r, h, w).transpose(0, 1, 4, 2, 5, 3).reshape(n, outc, h * r, w * r))


def case_bytes(seed, dtype, dims):
    """seeded bytes that hold -128 (0x80) and every other byte value at least once where the tensor has 256 elements or more; a smaller
    tensor holds as many DIFFERENT values as it has elements, 0x80, 0x7f, 0x00 and 0xff among them"""
    rng = np.random.default_rng(seed)
    size = int(np.prod(dims))
    must = np.array([0x80, 0x7f, 0x00, 0xff, 0x81, 0x01], np.uint8)
    rest = rng.permutation(np.setdiff1d(np.arange(256, dtype=np.uint8), must))
    vals = np.concatenate([must, rest])[:size]
    if size > 256:
        vals = np.concatenate([vals, rng.integers(0, 256, size=size - 256).astype(np.uint8)])
    return rng.permutation(vals).astype(np.uint8).view(tm2.NP_OF_DT[dtype]).reshape(dims)


def d2s_graph(dtype, dims, r, seed=5, in_q=None, out_q=None, out_dims=None, data_const=False, in_quant=None, out_quant=None):
    """data -> DepthToSpace(block_size r) -> output.  out_dims None: what the reference infers"""
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    in_q, out_q = in_q or IN_Q.get(dtype), out_q or OUT_Q.get(dtype)
    g = Graph(name="d2s_case")
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    if in_quant is not None:
        g.tensors[x].scales, g.tensors[x].zero_points = [f32(in_q[0])] * in_quant, [int(in_q[1])] * in_quant
    src = x
    if data_const:
        src = g.add_const("table", np.zeros(dims, tm2.NP_OF_DT[dtype]), dtype, *q(in_q))
    if out_dims is None:
        rr = max(1, r * r)
        out_dims = [dims[0], dims[1] // rr, dims[2] * r, dims[3] * r] if len(dims) == 4 else list(dims)
    y = g.add_tensor("out", list(out_dims), dtype, tm2.TT_VAR, None, *q(out_q))
    if out_quant is not None:
        g.tensors[y].scales, g.tensors[y].zero_points = [f32(out_q[0])] * out_quant, [int(out_q[1])] * out_quant
    g.output_nodes = [g.add_node("d2s", "DepthToSpace", [src], [y], block_size=r)]
    if dtype == DT_FP32:
        return g, np.random.default_rng(seed).normal(0, 1, size=dims).astype(np.float32)
    return g, case_bytes(seed, dtype, dims)


class SubPixel(ih.Neck):
    """interp_helpers.Neck with ReLU and DepthToSpace"""

    def relu(self):
        name = self._name("relu")
        y = self._var(name, self.dims(), self.quant(self.cur))
        self.last = self.g.add_node(name, "ReLU", [self.cur], [y], negative_slope=0.0)
        self.cur = y
        return y

    def d2s(self, r, out_q=None, src=None):
        x = self.cur if src is None else src
        n, c, h, w = self.dims(x)
        name = self._name("d2s")
        y = self._var(name, [n, c // (r * r), h * r, w * r], self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "DepthToSpace", [x], [y], block_size=r)
        self.cur = y
        return y

    def done_with(self, outputs, x):
        g, _ = self.done()
        g.output_nodes = list(outputs)
        return g, x


def espcn_tail(dtype, dims=(1, 8, 6, 6), r=2, outc=3, seed=81):
    """conv 3x3 -> ReLU -> conv 3x3 (outc * r * r channels) -> DepthToSpace: the node's output is the graph's"""
    c = SubPixel(seed, dtype, dims)
    c.conv(16, 3, 1); c.relu(); c.conv(outc * r * r, 3, 1); c.d2s(r)
    return c.done()


def edsr_upsampler(dtype, dims=(1, 8, 6, 6), r=2, seed=82, times=1):
    """conv 3x3 (C * r * r channels) -> DepthToSpace [-> the same again] -> conv 3x3"""
    c = SubPixel(seed, dtype, dims)
    for _ in range(times):
        c.conv(dims[1] * r * r, 3, 1); c.d2s(r)
    c.conv(3, 3, 1)
    return c.done()


def u8_into_concat(dims, r, lead, tail, seed=83):
    """uint8: Concat([lead planes, DepthToSpace(data), tail planes]) with every input at the Concat's parameters, so that the node writes
    its planes IN PLACE between neighbours on both sides, `lead` planes of OH * OW bytes into the Concat's image.  The neighbours are a
    1 x 1 convolution of data's first r * r ... channels -> nearest Interp x r, and they come first in node order: bytes the node wrote
    outside its own planes would stay wrong"""
    c = SubPixel(seed, DT_UINT8, dims, in_q=IN_Q[DT_UINT8])
    data = c.cur
    q = (0.04, 100)
    sides = []
    for ch in (lead, tail):
        c.conv(ch, 1, src=data)
        sides.append(c.interp(ih.by_scale(float(r)), out_q=q))
    mid = c.d2s(r, out_q=q, src=data)
    c.concat([sides[0], mid, sides[1]], q)
    return c.done_with([c.last], case_bytes(seed, DT_UINT8, dims))


def i8_source_is_a_concat_slice(seed=84, dims=(1, 8, 4, 4)):
    """int8: a (16 ch), b (32 ch) = convolutions of data; Concat([a, b]) -> conv; DepthToSpace r 2 reads b, which lies at channel 16 of the
    Concat's 48-channel pixels: c_off != 0 and a pixel stride wider than the source's channels"""
    c = SubPixel(seed, DT_INT8, dims)
    data = c.cur
    a = c.conv(16, 1, src=data)
    q = c.quant(a)
    b = c.conv(32, 3, 1, src=data)
    c.requant(b, q)
    c.concat([a, b], q)
    c.conv(8, 1)
    head = c.last
    c.d2s(2, out_q=(0.07, 0), src=b)
    return c.done_with([c.last, head], None)


def i8_into_multi_concat(cin, seed=85):
    """int8: Concat([DepthToSpace r 2 (data), Upsample-like Interp x2 of conv(data)]) at one scale, data (1, cin, 3, 3) holding -128.
    cin 64: the node's 16 channels are written in place into the Concat's buffer; cin 12: 3 channels, the Concat copies.  What the
    Concat of SEVERAL inputs makes of -128 is the reference's to say (the golden)"""
    dims = (1, cin, 3, 3)
    c = SubPixel(seed, DT_INT8, dims, in_q=IN_Q[DT_INT8])
    data = c.cur
    q = (0.05, 0)
    c.conv(cin // 4, 1, src=data)
    up = c.interp(ih.by_scale(2.0), out_q=q)
    mid = c.d2s(2, out_q=q, src=data)
    c.concat([mid, up], q)
    return c.done_with([c.last], case_bytes(seed, DT_INT8, dims))


# the single-node cases: id -> (type, input dims, block size).  What each is for is in tests/test_gpu_d2s.py
SINGLE = {
    "u8_rows_of_10": (DT_UINT8, (1, 4, 3, 5), 2),
    "u8_aligned_rows_of_48": (DT_UINT8, (1, 8, 8, 24), 2),
    "u8_r3_batch2": (DT_UINT8, (2, 18, 2, 7), 3),
    "u8_r4_one_pixel": (DT_UINT8, (1, 16, 1, 1), 4),
    "u8_r1_copy": (DT_UINT8, (1, 5, 3, 3), 1),
    "i8_outc3_padding": (DT_INT8, (1, 12, 3, 5), 2),
    "i8_outc16": (DT_INT8, (1, 64, 4, 4), 2),
    "i8_outc20_batch2": (DT_INT8, (2, 80, 2, 3), 2),
    "i8_r3": (DT_INT8, (1, 36, 2, 2), 3),
}


def _needs_input(build):
    def run():
        g, x = build()
        if x is None:
            d = g.tensors[g.nodes[g.input_nodes[0]].outputs[0]].dims
            x = case_bytes(7, DT_INT8, d)
            x[x == -128] = 5                             # (behind a convolution the byte never appears; keep the input the usual range)
        return g, x
    return run


def gpu_cases():
    """{id: (type, builder)}: every case the GPU tests run; a builder returns (graph, input)"""
    cases = {k: (dt, (lambda dt=dt, d=d, r=r: d2s_graph(dt, d, r))) for k, (dt, d, r) in SINGLE.items()}
    cases["u8_concat_slice"] = (DT_UINT8, lambda: u8_into_concat((1, 4, 2, 8), 2, 3, 2))            # planes of 64 bytes behind 3 of a neighbour
    cases["u8_concat_slice_odd_offset"] = (DT_UINT8, lambda: u8_into_concat((1, 18, 1, 1), 3, 1, 2))  # 2 planes of 9 bytes at byte 9
    cases["i8_source_concat_slice"] = (DT_INT8, _needs_input(i8_source_is_a_concat_slice))
    cases["i8_into_concat_in_place"] = (DT_INT8, lambda: i8_into_multi_concat(64))
    cases["i8_into_concat_copied"] = (DT_INT8, lambda: i8_into_multi_concat(12))
    for dt, tag in ((DT_INT8, "i8"), (DT_UINT8, "u8")):
        cases[tag + "_espcn_tail"] = (dt, lambda dt=dt: espcn_tail(dt))
        cases[tag + "_edsr_upsampler"] = (dt, lambda dt=dt: edsr_upsampler(dt))
    return cases


def form0_is_legal(case):
    """where TAMD_PIN=d2s_form=0 gives the canonical gather (plan_depthtospace): the node's output is ONE dense run -- every uint8 case
    here (the Concat cases have one image), and in int8 an output without padding channels that is no concat view"""
    if case.startswith("u8_"):
        return True
    return case in ("i8_outc16",)


# what runs when TAMD_PIN=d2s_form is not set (csrc/kernels.h: kD2sNewFormFromBytes; profiles/d2s.txt has the measurement): the new
# kernels from this many output bytes on, the gather below (where it is legal)
NEW_FORM_FROM_BYTES = 1 << 20


def default_form(dims):
    return 1 if int(np.prod(dims)) >= NEW_FORM_FROM_BYTES else 0


def expected_kernels(case, form):
    """the kernel of the node's one launch"""
    if form == 0 and form0_is_legal(case):
        return ["transpose_gather_q8"]
    if case == "u8_r1_copy":
        return ["slice_u8"]
    return ["d2s_u8" if case.startswith("u8_") else "d2s_i8"]


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


def _desc(dtype, dims, ttype=1, quant=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == 0 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def ask_d2s(dtype, in_dims, r, out_dims=None, const_input=False, in_quant=None, out_quant=None, with_param=True, inputs=1):
    """tamd_node_supported for a DepthToSpace node (dtype: the C ABI's code); out_dims None: what the reference infers"""
    p = capi.DepthToSpaceParam(int(r))
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_DEPTHTOSPACE, inputs, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    if out_dims is None:
        rr = max(1, r * r)
        out_dims = [in_dims[0], in_dims[1] // rr, in_dims[2] * r, in_dims[3] * r] if len(in_dims) == 4 else list(in_dims)
    outs = (lh.TensorDesc * 1)(_desc(dtype, out_dims, quant=out_quant))
    ins = (lh.TensorDesc * 2)(_desc(dtype, in_dims, 2 if const_input else 1, quant=in_quant), _desc(dtype, in_dims))
    return capi.lib().tamd_node_supported(C.byref(n), ins, inputs, outs, 1)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves): both are made before the device is touched"""
    return ih.library_output_shape(capi, tm_bytes)
