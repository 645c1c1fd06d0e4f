"""Builders for the tests of the uint8 Crop node (tests/test_crop_cpu.py, tests/test_gpu_crop.py): a Crop alone, nearest Interp -> Crop,
the top-down merge Interp -> Crop -> Eltwise and RetinaFace's pyramid block.  Every case is tmfile bytes with explicit quantisation
parameters: the reference library and the device read the same model.  A Crop reads of its second input the shape alone, so the
single-node cases hand it a constant of that shape; the merges hand it the lateral itself, as RetinaFace does.

    python tests/crop_helpers.py          writes tests/golden/crop_cases.npz (needs oracle/_ref/libtengine-lite.so)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import interp_helpers as ih  # noqa: E402
import lut_helpers as lh  # noqa: E402
from tengine_amd import capi, tm2  # noqa: E402
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "crop_cases.npz")
OP_CROP = 30            # TAMD_OP_CROP
f32 = lh.f32
digest, equals_golden = ih.digest, ih.equals_golden
DIGEST_ONLY = {"ragged_blocks"}               # 13 KB of random bytes: the golden holds their shape and SHA-256
IN_Q, OUT_Q = (0.05, 77), (0.031, 12)
CAFFE2, CAFFE1, MXNET2 = dict(flag=0, axis=2), dict(flag=0, axis=1), dict(flag=1, axis=2, num_args=2)


def box_start(p):
    """where the box starts on (C, H, W): crop_ref.c:147-253"""
    return (p.get("offset_c", 0) if p.get("flag", 0) == 0 and p.get("axis", 2) == 1 else 0, p.get("offset_h", 0), p.get("offset_w", 0))


def numpy_crop(x, like_dims, p):
    c0, h0, w0 = box_start(p)
    n, c, h, w = like_dims
    return x[:n, c0:c0 + c, h0:h0 + h, w0:w0 + w]


def crop_graph(in_dims, like_dims, p, in_q=IN_Q, out_q=OUT_Q, seed=5, dtype=DT_UINT8, out_dims=None, like_const=True, data_const=False, in_quant=None):
    """data -> Crop(data, like) -> output; `like` a zero constant of like_dims (or a second graph input); out_dims None: like_dims"""
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    g = Graph(name="crop_case")
    x = g.add_input("data", list(in_dims), dtype, *q(in_q))
    if in_quant is not None:
        g.tensors[x].scales, g.tensors[x].zero_points = [f32(in_q[0])] * in_quant, [int(in_q[1])] * in_quant
    src = x
    if data_const:
        src = g.add_const("table", np.zeros(in_dims, tm2.NP_OF_DT[dtype]), dtype, *q(in_q))
    if like_const:
        like = g.add_const("like", np.zeros(like_dims, tm2.NP_OF_DT[dtype]), dtype, *q(in_q))
    else:
        like = g.add_input("like", list(like_dims), dtype, *q(in_q))
    y = g.add_tensor("out", list(like_dims if out_dims is None else out_dims), dtype, tm2.TT_VAR, None, *q(out_q))
    g.output_nodes = [g.add_node("crop", "Crop", [src, like], [y], **p)]
    if dtype == DT_FP32:
        return g, np.random.default_rng(seed).normal(0, 1, size=in_dims).astype(np.float32)
    return g, lh.random_bytes(seed, dtype, in_dims)


class Pyramid(ih.Neck):
    """interp_helpers.Neck with Crop and the four same-shape Eltwise types"""

    def crop(self, like, p, out_q=None, src=None, like_dims=None):
        x = self.cur if src is None else src
        if like_dims is not None:
            like = self.g.add_const(self._name("like"), np.zeros(like_dims, tm2.NP_OF_DT[self.dtype]), self.dtype, *self._q(self.quant(x) or (1.0, 0)))
        name = self._name("crop")
        y = self._var(name, self.dims(like), self.quant(x) if out_q is None else out_q)
        self.last = self.g.add_node(name, "Crop", [x, like], [y], **p)
        self.cur = y
        return y

    def eltwise(self, kind, a, b, out_q=None):
        name = self._name("elt")
        q = None if self.dtype == DT_FP32 else (out_q or (self.scale(a) * 1.4, 0 if self.dtype == DT_INT8 else 120))
        y = self._var(name, self.dims(a if np.prod(self.dims(a)) >= np.prod(self.dims(b)) else b), q)
        self.last = self.g.add_node(name, "Eltwise", [a, b], [y], type=kind, caffe_flavor=1)
        self.cur = y
        return y

    def done2(self, outputs, seed=1, force=True):
        """several graph outputs; the input holds bytes 0 and 255 for certain"""
        g, x = self.done(seed)
        g.output_nodes = list(outputs)
        if force and self.dtype == DT_UINT8:
            x.reshape(-1)[::max(1, x.size // 9)] = 0
            x.reshape(-1)[1::max(1, x.size // 9)] = 255
        return g, x


def chain_graph(dims=(1, 8, 8, 10), scale=2.0, cut=(15, 20), off=(0, 0), in_q=IN_Q, mid_q=OUT_Q, out_q=(0.043, 140), second=None, seed=71):
    """data -> Interp(nearest, scale) -> Crop to `cut` from `off`.  mid_q == in_q: the Interp's byte map is the identity.  second: the
    (cut, off) of a second Crop that reads the same Interp (both are graph outputs)"""
    c = Pyramid(seed, DT_UINT8, dims, in_q=in_q)
    up = c.interp(ih.by_scale(scale), out_q=mid_q)
    c.crop(None, dict(CAFFE2, offset_h=off[0], offset_w=off[1]), out_q=out_q, like_dims=[dims[0], dims[1], cut[0], cut[1]])
    outs = [c.last]
    if second:
        c.crop(None, dict(CAFFE2, offset_h=second[1][0], offset_w=second[1][1]), out_q=out_q, src=up, like_dims=[dims[0], dims[1], second[0][0], second[0][1]])
        outs.append(c.last)
    return c.done2(outs, force=False)


# three (lateral, Interp output, Crop output, Eltwise output) parameter sets
QSETS = {
    "a": ((0.05, 77), (0.031, 12), (0.043, 140), (0.09, 100)),
    "b": ((0.02, 128), (0.02, 128), (0.02, 128), (0.035, 128)),          # the Interp's map is the identity
    "c": ((0.017, 3), (0.029, 250), (0.011, 60), (0.012, 131)),          # zero points near both ends; results saturate at 0 and at 255
}


def topdown_graph(dims=(1, 4, 15, 20), kind=tm2.ELT_SUM, crop_first=False, qset="a", off=(0, 0), seed=72, form="fused"):
    """data (N, C, OH, OW) is the lateral; small = every second pixel of it (max-pool 1 x 1, stride 2) -> Interp x2 -> Crop(like = data)
    -> Eltwise with the lateral, the cropped operand listed first or second.  form: "fused" as above; "cut_channels": the lateral is a
    1 x 1 convolution to C - 1 channels and the caffe axis-1 Crop drops channel 0; "gate": the Eltwise is PROD with a (N, C, 1, 1) gate
    (dims square); "second_reader": a Sigmoid reads the Crop's output too"""
    ql, qi, qc, qo = QSETS[qset]
    c = Pyramid(seed, DT_UINT8, dims, in_q=ql)
    data = c.cur
    lat, p = data, dict(CAFFE2, offset_h=off[0], offset_w=off[1])
    if form == "cut_channels":
        lat, p = c.conv(dims[1] - 1, 1, src=data), dict(CAFFE1, offset_c=1, offset_h=off[0], offset_w=off[1])
    if form == "gate":
        assert dims[2] == dims[3]
        lat = c.pool(dims[2], dims[2], src=data)
    c.pool(1, 2, src=data)
    c.interp(ih.by_scale(2.0), out_q=qi)
    cut = c.crop(lat if form != "gate" else data, p, out_q=qc)
    outs = []
    if form == "second_reader":
        c.act("Sigmoid")
        outs.append(c.last)
    c.eltwise(kind, *((cut, lat) if crop_first else (lat, cut)), out_q=qo)
    return c.done2(outs + [c.last])


def pyramid_graph(dtype=DT_UINT8, dims=(1, 16, 15, 20), seed=73, crop=CAFFE2):
    """RetinaFace's top-down merge: lateral = conv1x1(data) (1, 16, 15, 20); data -> every second pixel -> conv1x1 (1, 16, 8, 10) -> Interp
    x2 -> Crop(like = lateral) -> Eltwise SUM(lateral, .) -> conv3x3"""
    c = Pyramid(seed, dtype, dims)
    data = c.cur
    lat = c.conv(dims[1], 1, src=data)
    c.pool(1, 2, src=data)
    c.conv(dims[1], 1)
    c.interp(ih.by_scale(2.0))
    cut = c.crop(lat, dict(crop))
    c.eltwise(tm2.ELT_SUM, lat, cut)
    c.conv(dims[1], 3, 1)
    return c.done()


# the single-node cases: id -> (in dims, like dims, param).  What each is for is in tests/test_gpu_crop.py
SINGLE = {
    "retina_cut": ((1, 8, 16, 20), (1, 8, 15, 20), dict(CAFFE2)),
    "offsets_hw": ((1, 8, 16, 20), (1, 8, 14, 17), dict(CAFFE2, offset_h=1, offset_w=2)),
    "caffe_axis1_c3": ((1, 8, 6, 7), (1, 5, 5, 6), dict(CAFFE1, offset_c=3, offset_h=1, offset_w=1)),
    "axis2_ignores_offset_c": ((1, 8, 6, 7), (1, 5, 5, 6), dict(CAFFE2, offset_c=3, offset_h=1, offset_w=1)),
    "mxnet_args2": ((1, 4, 9, 11), (1, 4, 7, 8), dict(MXNET2, offset_c=2, offset_h=1, offset_w=2)),
    "whole_input": ((1, 3, 5, 7), (1, 3, 5, 7), dict(CAFFE2)),
    "no_aligned_row": ((1, 3, 5, 7), (1, 3, 4, 5), dict(CAFFE2, offset_h=1, offset_w=1)),
    "batch2": ((2, 4, 8, 10), (2, 4, 7, 9), dict(CAFFE2, offset_h=1)),
    "ragged_blocks": ((2, 5, 37, 41), (2, 5, 33, 40), dict(CAFFE2, offset_h=2, offset_w=1)),
}
CHAINS = {
    "chain_x2_identity_map": lambda: chain_graph(mid_q=IN_Q),
    "chain_x2_off11": lambda: chain_graph(cut=(15, 19), off=(1, 1)),
    "chain_scale15": lambda: chain_graph(scale=1.5, cut=(11, 13), off=(1, 2)),
    "chain_batch2": lambda: chain_graph(dims=(2, 3, 8, 10), cut=(15, 19), off=(0, 1)),
    "chain_second_reader": lambda: chain_graph(second=((14, 18), (2, 1))),
}
KINDS = {"prod": tm2.ELT_PROD, "sum": tm2.ELT_SUM, "sub": tm2.ELT_SUB, "max": tm2.ELT_MAX}
TOPDOWN = {}
for _k, _v in KINDS.items():
    for _first in (False, True):
        TOPDOWN["td_%s_%s" % (_k, "first" if _first else "second")] = (lambda v=_v, f=_first, k=_k: topdown_graph(kind=v, crop_first=f, qset="a" if k in ("sum", "sub") else "b"))
TOPDOWN["td_w19_c3_offset"] = lambda: topdown_graph(dims=(1, 3, 15, 19), kind=tm2.ELT_SUB, crop_first=True, qset="c", off=(1, 1))
TOPDOWN["td_batch2_ragged"] = lambda: topdown_graph(dims=(2, 5, 15, 19), kind=tm2.ELT_SUM, qset="a", off=(0, 1))
TOPDOWN["td_saturating"] = lambda: topdown_graph(kind=tm2.ELT_PROD, qset="c")
# maps narrower than 16: every chunk walks byte by byte, several rows per chunk, and the row and plane wraps inside the walk feed later gathers
TOPDOWN["td_narrow_batch2_offset"] = lambda: topdown_graph(dims=(2, 3, 7, 9), kind=tm2.ELT_SUB, crop_first=True, qset="a", off=(1, 1))
TOPDOWN["td_tiny_planes"] = lambda: topdown_graph(dims=(1, 3, 3, 5), kind=tm2.ELT_SUM, qset="c", off=(1, 1))          # a plane is 15 bytes: a chunk holds two plane crossings
TOPDOWN["td_wide_rows"] = lambda: topdown_graph(dims=(1, 1, 2, 520), kind=tm2.ELT_MAX, qset="a")                     # OW > 512: the column indices are read from memory, not LDS
NOT_FUSED = {
    "nf_cut_channels": lambda: topdown_graph(form="cut_channels"),
    "nf_gate": lambda: topdown_graph(dims=(1, 4, 15, 15), kind=tm2.ELT_PROD, crop_first=True, form="gate"),
    "nf_second_reader": lambda: topdown_graph(form="second_reader"),
}


def gpu_cases():
    """{id: builder}: every uint8 case the GPU tests run; a builder returns (graph, input)"""
    cases = {k: (lambda v=v: crop_graph(*v)) for k, v in SINGLE.items()}
    for d in (CHAINS, TOPDOWN, NOT_FUSED):
        cases.update(d)
    cases["pyramid"] = pyramid_graph
    return cases


def reference_outputs(ref, g, x, dtype=DT_UINT8):
    return ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))


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


def write_golden(ref):
    """records tests/golden/crop_cases.npz from the real reference library: every GPU case on its seeded input"""
    z = {}
    for case, build in sorted(gpu_cases().items()):
        g, x = build()
        z.update(golden_entry(case, reference_outputs(ref, g, x)))
    np.savez_compressed(GOLDEN, **z)
    return os.path.getsize(GOLDEN), len(z)


def _desc(dtype, dims, ttype=1, quant=None, keep=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == DT_FP32 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def ask_crop(dtype, in_dims, like_dims, p, out_dims=None, const_input=False, in_quant=None, out_quant=None, with_param=True, inputs=2):
    """tamd_node_supported for a Crop node; out_dims None: what the reference infers (input 1's)"""
    q = capi.CropParam(*[int(p.get(k, 2 if k == "axis" else 0)) for k in tm2.CROP_FIELDS])
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_CROP, inputs, 1
    if with_param:
        n.param = C.cast(C.pointer(q), C.c_void_p)
    outs = (lh.TensorDesc * 1)(_desc(dtype, like_dims if out_dims is None else out_dims, quant=out_quant))
    ins = (lh.TensorDesc * 2)(_desc(dtype, in_dims, 2 if const_input else 1, quant=in_quant), _desc(dtype, like_dims))
    return capi.lib().tamd_node_supported(C.byref(n), ins, inputs, outs, 1)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves): both are made before the device is touched"""
    return ih.library_output_shape(capi, tm_bytes)


if __name__ == "__main__":
    from oracle import ref_capi
    assert ref_capi.available(), "build the reference library first (oracle/build_ref.py)"
    print(GOLDEN, *write_golden(ref_capi))
