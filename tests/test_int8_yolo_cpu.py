"""int8 YOLOv3-tiny whole on the device, the parts that need no GPU: what the support queries answer for an int8 Upsample, where the
plugin's splitter puts the graph (ONE "HIP" subgraph since the int8 Upsample runs on the device), the committed calibration table
and the committed golden against the real reference."""
import ctypes as C
import json
import os

import numpy as np

from tengine_amd import capi, models, tm2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "yolov3_tiny_int8_416_seed3.npz")


class _T(C.Structure):          # tamd_tensor_desc
    _fields_ = [("dtype", C.c_int), ("ttype", C.c_int), ("dim_num", C.c_int), ("dims", C.c_int * 8), ("data", C.c_void_p),
                ("quant_num", C.c_int), ("scales", C.c_void_p), ("zero_points", C.c_void_p), ("name", C.c_char_p)]


class _N(C.Structure):          # tamd_node_desc
    _fields_ = [("op", C.c_int), ("input_num", C.c_int), ("inputs", C.c_void_p), ("output_num", C.c_int), ("outputs", C.c_void_p),
                ("param", C.c_void_p), ("name", C.c_char_p)]


def _t(dtype, dims, ttype=1):
    d = _T()
    d.dtype, d.ttype, d.dim_num, d.quant_num = dtype, ttype, len(dims), 0 if dtype == 0 else 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    return d


def _ask_upsample(dtype, in_dims, out_dims, scale):
    L = capi.lib()
    n = _N()
    n.op, n.input_num, n.output_num = 9, 1, 1            # TAMD_OP_UPSAMPLE
    p = C.c_float(scale)
    n.param = C.cast(C.pointer(p), C.c_void_p)
    return L.tamd_node_supported(C.byref(n), (_T * 1)(_t(dtype, in_dims)), 1, (_T * 1)(_t(dtype, out_dims)), 1)


def test_node_supported_answers_for_upsample():
    F32, I8, U8 = 0, 2, 3
    L = capi.lib()
    assert [L.tamd_op_supported(9, dt) for dt in (F32, I8, U8)] == [1, 1, 1]
    assert _ask_upsample(I8, [1, 16, 4, 4], [1, 16, 8, 8], 2.0) == 1
    assert _ask_upsample(I8, [2, 5, 3, 4], [2, 5, 9, 12], 3.0) == 1
    assert _ask_upsample(I8, [1, 16, 4, 4], [1, 16, 6, 6], 1.5) == 0           # a fractional factor: the reference truncates out / scale per pixel
    assert _ask_upsample(I8, [1, 16, 4, 4], [1, 16, 2, 2], 0.5) == 0
    assert _ask_upsample(I8, [16, 4, 4], [16, 8, 8], 2.0) == 0                 # int8 tensors are NHWC on the device: 4-D only
    assert _ask_upsample(I8, [1, 16], [1, 16], 1.0) == 0
    for dt in (U8, F32):                                                       # unchanged: the integer-factor rule alone
        assert _ask_upsample(dt, [1, 16, 4, 4], [1, 16, 8, 8], 2.0) == 1
        assert _ask_upsample(dt, [1, 16, 4, 4], [1, 16, 6, 6], 1.5) == 0
        assert _ask_upsample(dt, [16, 4, 4], [16, 8, 8], 2.0) == 1


def test_int8_yolov3_tiny_is_one_hip_subgraph(ref):
    """the splitter's placement (computed even where the device pre_run then fails for lack of a GPU): every operator of the int8
    graph in ONE "HIP" subgraph, nothing left to the CPU device -- the Upsample used to cut it in three"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g = models.build("yolov3_tiny", "int8", 1, res=64)
    pl = tp._split_only(ref, g, models.synth_input(g, 3), ref.MODE_INT8)
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert len(real) == 1 and real[0][0] == "HIP", pl
    ops = [o for o in real[0][1] if o not in ("InputOp", "Const")]
    assert len(ops) == 35 and ops.count("Upsample") == 1 and ops.count("Convolution") == 13 and ops.count("Pooling") == 6, pl
    assert sum(r for dev, _, r, _ in pl if dev != "HIP") == 0, pl


def test_committed_calibration_table_reproduces_the_int8_model():
    """tengine_amd/calib/yolov3_tiny_int8.json (models.calib_table(.., write=True)) names every activation of the builder's graph,
    models.build takes its scales from it -- bit-identical on every host -- and a calibration run here lands on the same numbers up
    to the fp32 forward's summation order; the Upsample's input and output scales differ (no sharing: the rescaling case is the
    real one)"""
    path = os.path.join(models.CALIB_DIR, "yolov3_tiny_int8.json")
    assert os.path.exists(path)
    table = json.load(open(path))
    gf = models.yolov3_tiny_fp32()
    names = {t.name for t in gf.tensors if t.ttype == tm2.TT_VAR}
    assert names == set(table)
    g = models.build("yolov3_tiny", "int8")
    want = models.quantize_int8(gf, table=table)
    assert tm2.write_tm2(g) == tm2.write_tm2(want)
    up = [n for n in g.nodes if n.op == "Upsample"]
    assert len(up) == 1
    s_in, s_out = g.tensors[up[0].inputs[0]].scales[0], g.tensors[up[0].outputs[0]].scales[0]
    assert s_in == float(np.float32(table[g.tensors[up[0].inputs[0]].name] / 127.0)) and s_in != s_out
    route = [n for n in g.nodes if n.op == "Concat" and len(n.inputs) == 2][0]
    assert s_out == g.tensors[route.outputs[0]].scales[0]          # concat inputs carry the concat's scale: written in place
    fresh = models.calibrate_absmax(gf)
    for k, v in table.items():
        assert abs(fresh[k] - v) <= 1e-3 * abs(v), (k, fresh[k], v)


def test_golden_is_the_real_reference(ref):
    """tests/golden/yolov3_tiny_int8_416_seed3.npz (make_golden_yolov3_tiny_int8.py) == the reference CPU device, run here"""
    g = models.build("yolov3_tiny", "int8", 1)
    x = models.synth_input(g, 3)
    outs = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8, min(16, os.cpu_count() or 1))
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == ["out0", "out1"] and len(outs) == 2
    for i, o in enumerate(outs):
        w = gold["out%d" % i]
        assert w.dtype == np.int8 and w.shape == o.shape == [(1, 255, 13, 13), (1, 255, 26, 26)][i]
        assert np.array_equal(w, o)
        assert len(np.unique(w)) > 100
