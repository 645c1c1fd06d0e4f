"""uint8 Crop on the device, the parts that need no GPU: crop_refusal's answers (every accepted and refused form, each refusal by its
name), the support queries, shape inference against the reference's, the tmfile writer and reader, where the plugin's splitter puts
the node, and the committed golden against the reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import crop_helpers as ch
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3
G = ch.crop_graph
X, LIKE = (1, 8, 16, 20), (1, 8, 15, 20)

# (what is asked, the words of the refusal): dims of the data, dims of input 1, parameter, and what else differs from a node that runs
REFUSED = [
    ("centre_crop", X, (1, 8, 12, 12), dict(flag=1, num_args=1, crop_h=12, crop_w=12), {}, "centre crop"),
    ("flag_2", X, LIKE, dict(flag=2), {}, "a flag other than 0"),
    ("flag_negative", X, LIKE, dict(flag=-1), {}, "a flag other than 0"),
    ("mxnet_args0", X, LIKE, dict(flag=1, num_args=0), {}, "num_args 2 only"),
    ("mxnet_args3", X, LIKE, dict(flag=1, num_args=3), {}, "num_args 2 only"),
    ("caffe_axis0", X, LIKE, dict(flag=0, axis=0), {}, "axis 1 or 2 only"),
    ("caffe_axis3", X, LIKE, dict(flag=0, axis=3), {}, "axis 1 or 2 only"),
    ("negative_offset_h", X, LIKE, dict(ch.CAFFE2, offset_h=-1), {}, "negative offset"),
    ("negative_offset_w", X, LIKE, dict(ch.MXNET2, offset_w=-2), {}, "negative offset"),
    ("negative_offset_c", X, (1, 5, 15, 20), dict(ch.CAFFE1, offset_c=-1), {}, "negative offset"),
    ("box_leaves_h", X, LIKE, dict(ch.CAFFE2, offset_h=2), {}, "leaves the data tensor"),
    ("box_leaves_w", X, LIKE, dict(ch.MXNET2, offset_w=1), {}, "leaves the data tensor"),
    ("box_leaves_c", X, (1, 6, 15, 20), dict(ch.CAFFE1, offset_c=3), {}, "leaves the data tensor"),
    ("like_has_more_channels", X, (1, 9, 15, 20), dict(ch.CAFFE2), {}, "leaves the data tensor"),
    ("like_is_larger", X, (1, 8, 17, 20), dict(ch.CAFFE2), {}, "leaves the data tensor"),
    ("batch_differs", (2, 8, 16, 20), LIKE, dict(ch.CAFFE2), {}, "same batch"),
    ("batch_differs_more", X, (2, 8, 15, 20), dict(ch.CAFFE2), {}, "same batch"),
    ("data_3d", (8, 16, 20), (8, 15, 20), dict(ch.CAFFE2), {}, "4-D tensors only"),
    ("like_2d", X, (15, 20), dict(ch.CAFFE2), dict(out_dims=list(LIKE)), "4-D tensors only"),
    ("per_channel", X, LIKE, dict(ch.CAFFE2), dict(in_quant=8), "per-tensor"),
    ("int8", X, LIKE, dict(ch.CAFFE2), dict(dtype=DT_INT8, in_q=(0.05, 0), out_q=(0.05, 0)), "uint8 graphs only"),
    ("fp32", X, LIKE, dict(ch.CAFFE2), dict(dtype=DT_FP32), "uint8 graphs only"),
]


def _error(g):
    return ch.library_outcome(tm2.write_tm2(g))[1]


@pytest.mark.parametrize("case", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_forms_are_refused_by_name_when_a_file_carries_them(case):
    """through the tmfile reader and prerun's shape inference / validation, which run before the device is touched"""
    _, x, like, p, kw, words = case
    assert words in _error(G(x, like, p, **kw)[0]), _error(G(x, like, p, **kw)[0])


def test_a_constant_data_input_is_refused_and_a_node_that_runs_gets_as_far_as_the_device():
    assert "must not be a constant" in _error(G(X, LIKE, dict(ch.CAFFE2), data_const=True)[0])
    for case, (x, like, p) in ch.SINGLE.items():
        assert "crop" not in _error(G(x, like, p)[0]).lower(), case


def test_support_queries():
    L = capi.lib()
    A = ch.ask_crop
    assert ch.OP_CROP == capi.OP_CROP == 30
    assert [L.tamd_op_supported(30, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 1]
    # what runs: every single-node case of the GPU tests
    for case, (x, like, p) in ch.SINGLE.items():
        assert A(U8, x, like, p) == 1, case
    assert A(U8, X, LIKE, dict(flag=0, axis=2, num_args=7, crop_h=3, crop_w=3, center_crop=1)) == 1       # fields the caffe form does not read
    # .. and what does not, each as the rule says
    for name, x, like, p, kw, _ in REFUSED:
        dt = {DT_INT8: I8, DT_FP32: F32}.get(kw.get("dtype"), U8)
        assert A(dt, x, like, p, out_dims=kw.get("out_dims"), in_quant=kw.get("in_quant")) == 0, name
    assert A(U8, X, LIKE, dict(ch.CAFFE2), out_dims=[1, 8, 16, 20]) == 0 and A(U8, X, LIKE, dict(ch.CAFFE2), out_dims=[8, 15, 20]) == 0       # (a file's own output dims are inferred anew)
    assert A(U8, X, LIKE, dict(ch.CAFFE2), out_quant=8) == 0
    assert A(U8, X, LIKE, dict(ch.CAFFE2), const_input=True) == 0
    assert A(U8, X, LIKE, dict(ch.CAFFE2), with_param=False) == 0
    assert A(U8, X, LIKE, dict(ch.CAFFE2), inputs=1) == 0
    assert A(FP16, X, LIKE, dict(ch.CAFFE2)) == 0
    # the operators that were there keep their answers and their codes; 21, 24, 27 and 29 are reserved, never-supported values
    assert [L.tamd_op_supported(op, I8) for op in range(29)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1]
    assert [L.tamd_op_supported(op, U8) for op in range(29)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1]
    assert [L.tamd_op_supported(op, F32) for op in range(29)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert [L.tamd_op_supported(29, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]
    assert [L.tamd_op_supported(31, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]


# what crop_refusal answers (tests/csrc/crop_rules_check.cc): (input line, expected output line).  The line's fields: dtype has_param
# inputs const in_quant out_quant | rank and dims of the data | of input 1 | the nine parameter fields | rank and dims of the output
P2, P1, PM = "0 0 %d %d 0 0 0 2 0", "0 %d %d %d 0 0 0 1 0", "2 %d %d %d 0 0 0 2 1"
RULES = [
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "OK start=0,0,0,0 out=1,8,15,20"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (1, 0), "OK start=0,0,1,0 out=1,8,15,20"),                       # the last row that fits
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 14 17 " + P2 % (2, 3), "OK start=0,0,2,3 out=1,8,14,17"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 5 14 17 " + P1 % (3, 2, 3), "OK start=0,3,2,3 out=1,5,14,17"),                     # axis 1: offset_c counts
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 5 14 17 0 3 2 3 0 0 0 2 0", "OK start=0,0,2,3 out=1,5,14,17"),                     # axis 2: it does not
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 5 14 17 " + PM % (3, 2, 3), "OK start=0,0,2,3 out=1,5,14,17"),                     # MXNet: neither
    ("u8 1 2 0 1 1 4 2 3 5 7 4 2 3 5 7 " + P2 % (0, 0), "OK start=0,0,0,0 out=2,3,5,7"),                              # the whole input
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0) + " 4 1 8 15 20", "OK start=0,0,0,0 out=1,8,15,20"),       # the output's dims given, and right
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0) + " 4 1 8 16 20", "REFUSED Crop: the output does not have the dims the reference infers"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0) + " 3 8 15 20", "REFUSED Crop: the output does not have the dims the reference infers"),
    ("u8 0 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "REFUSED Crop needs its parameter"),
    ("i8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "REFUSED Crop runs on the device in uint8 graphs only"),
    ("f32 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "REFUSED Crop runs on the device in uint8 graphs only"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 12 12 1 0 0 0 12 12 1 2 1", "REFUSED the centre crop (MXNet form, num_args 1) does not run on the device"),
    ("u8 1 1 0 1 1 4 1 8 16 20 0 1 0 0 0 12 12 1 2 1", "REFUSED the centre crop (MXNet form, num_args 1) does not run on the device"),       # .. and it has no input 1
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 0 0 0 0 0 0 0 2 2", "REFUSED Crop: a flag other than 0 (caffe) and 1 (MXNet) has no kernel in the reference"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 3 0 0 0 0 0 0 2 1", "REFUSED Crop: the MXNet form runs with num_args 2 only"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 0 0 0 0 0 0 0 3 0", "REFUSED Crop: the caffe form runs with axis 1 or 2 only"),
    ("u8 1 1 0 1 1 4 1 8 16 20 0 " + P2 % (0, 0), "REFUSED Crop takes two inputs: the data and the tensor whose shape it takes"),
    ("u8 1 2 0 1 1 3 8 16 20 3 8 15 20 " + P2 % (0, 0), "REFUSED Crop runs on the device on 4-D tensors only"),
    ("u8 1 2 0 1 1 4 1 8 16 20 2 15 20 " + P2 % (0, 0), "REFUSED Crop runs on the device on 4-D tensors only"),
    ("u8 1 2 1 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "REFUSED Crop: the data input must not be a constant"),
    ("u8 1 2 0 8 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "REFUSED Crop needs per-tensor quant params on the data and the output"),
    ("u8 1 2 0 1 8 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 0), "REFUSED Crop needs per-tensor quant params on the data and the output"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (-1, 0), "REFUSED Crop: a negative offset does not run on the device"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 5 15 20 " + P1 % (-2, 0, 0), "REFUSED Crop: a negative offset does not run on the device"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 5 15 20 0 -2 0 0 0 0 0 2 0", "OK start=0,0,0,0 out=1,5,15,20"),                    # axis 2 never reads offset_c
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (2, 0), "REFUSED Crop: the box leaves the data tensor"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (0, 1), "REFUSED Crop: the box leaves the data tensor"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 9 15 20 " + P2 % (0, 0), "REFUSED Crop: the box leaves the data tensor"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 6 15 20 " + P1 % (3, 0, 0), "REFUSED Crop: the box leaves the data tensor"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 15 20 " + P2 % (2147483647, 0), "REFUSED Crop: the box leaves the data tensor"),  # no overflow on the way
    ("u8 1 2 0 1 1 4 1 8 16 20 4 2 8 15 20 " + P2 % (0, 0), "REFUSED Crop: the two inputs must have the same batch"),
    ("u8 1 2 0 1 1 4 1 8 16 20 4 1 8 0 20 " + P2 % (0, 0), "REFUSED Crop: every dimension must be at least 1"),
]


def test_crop_refusal_names_every_refusal_and_resolves_the_box(tmp_path):
    """the rule itself, as a stand-alone host program (its own main, host code only) under the address and undefined-behaviour sanitizers"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "crop_rules_check")
    subprocess.check_call([hipcc, "-std=c++17", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tengine_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "crop_rules_check.cc"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], input="\n".join(r[0] for r in RULES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(RULES), out.stdout
    for (case, want), got in zip(RULES, lines):
        assert got == want, (case, got, want)
    assert len({w for _, w in RULES if w.startswith("REFUSED")}) >= 14           # every refusal has its own reason


# (id, data dims, dims of input 1, parameter): what crop.c:34-78 infers
SHAPES = [(k,) + v for k, v in ch.SINGLE.items()]


@pytest.mark.parametrize("case", SHAPES, ids=[s[0] for s in SHAPES])
def test_inferred_shape_is_the_references(ref, case):
    """a file whose output tensor carries NO useful shape: what the reference infers is what the library infers (input 1's dims), and
    the bytes the reference computes are the data's own, whatever the two tensors' parameters"""
    _, x_dims, like, p = case
    g, x = G(x_dims, like, p)
    g.tensors[g.nodes[g.output_nodes[0]].outputs[0]].dims = [1, 1, 1, 1]
    b = tm2.write_tm2(g)
    out = ch.reference_outputs(ref, g, x)[0]
    shape, err = ch.library_outcome(b)
    assert shape == out.shape == tuple(like), (shape, out.shape, err)
    assert "crop" not in err.lower(), err
    assert np.array_equal(out, ch.numpy_crop(x, like, p))


def test_writer_and_reader_round_trip_the_nine_fields():
    p = dict(num_args=2, offset_c=3, offset_h=4, offset_w=5, crop_h=6, crop_w=7, center_crop=1, axis=1, flag=1)
    g, _ = G(X, LIKE, p)
    b = tm2.write_tm2(g)
    node = [n for n in tm2.read_tm2(b).nodes if n.op == "Crop"]
    assert len(node) == 1 and node[0].params == p and len(node[0].inputs) == 2
    g, _ = G(X, LIKE, {})                                # the defaults are crop.c's init_op
    assert [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "Crop"][0].params == dict(zip(tm2.CROP_FIELDS, (0, 0, 0, 0, 0, 0, 0, 2, 0)))
    # the C ABI's reader reads the same blob: the bool is one byte, axis sits behind its padding -- an axis-1 Crop keeps its channel offset
    g, _ = G((1, 8, 6, 7), (1, 5, 5, 6), dict(ch.CAFFE1, offset_c=3, offset_h=1, offset_w=1, center_crop=1))
    shape, err = ch.library_outcome(tm2.write_tm2(g))
    assert shape == (1, 5, 5, 6) and "crop" not in err.lower(), err
    g, _ = G((1, 8, 6, 7), (1, 6, 5, 6), dict(ch.CAFFE1, offset_c=3, offset_h=1, offset_w=1))
    assert "leaves the data tensor" in _error(g)
    g, _ = G((1, 8, 6, 7), (1, 6, 5, 6), dict(ch.CAFFE2, offset_c=3, offset_h=1, offset_w=1))
    assert "crop" not in _error(g).lower()


def test_a_file_with_a_crop_loads_through_the_c_abi():
    L = capi.lib()
    for build in (lambda: G(X, LIKE, dict(ch.CAFFE2)), ch.pyramid_graph):
        b = tm2.write_tm2(build()[0])
        h = L.tamd_graph_load_tm2(b, len(b))
        assert h, L.tamd_last_error()
        L.tamd_graph_destroy(h)


@pytest.mark.parametrize("case", ["retina_cut", "caffe_axis1_c3", "mxnet_args2", "chain_scale15", "td_sub_first", "nf_gate", "pyramid"])
def test_written_tmfile_runs_in_the_reference(ref, case):
    """the reference loads a file tm2.py wrote and runs it; the shape it infers is the one the library infers"""
    g, x = ch.gpu_cases()[case]()
    out = ch.reference_outputs(ref, g, x)
    assert len(out) == len(g.output_nodes) and out[0].dtype == np.uint8
    shape, err = ch.library_outcome(tm2.write_tm2(g))
    assert shape == out[0].shape, (shape, out[0].shape, err)
    assert "not supported" not in err and "crop" not in err.lower(), err


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


def test_plugin_keeps_the_pyramid_block_in_one_hip_subgraph(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ch.pyramid_graph(DT_UINT8)
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert len(real) == 1 and real[0][0] == "HIP" and {"Crop", "Interp", "Eltwise", "Convolution"} <= set(real[0][1]), real


@pytest.mark.parametrize("dtype", [DT_INT8, DT_FP32])
def test_plugin_leaves_the_crop_of_int8_and_fp32_graphs_to_the_cpu_device(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ch.pyramid_graph(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    crops = [(dev, ops) for dev, ops in real if "Crop" in ops]
    assert len(crops) == 1 and crops[0][0] != "HIP", real
    i = real.index(crops[0])
    assert 0 < i < len(real) - 1 and any(dev == "HIP" for dev, _ in real[:i]) and any(dev == "HIP" for dev, _ in real[i + 1:]), real


def test_plugin_leaves_a_refused_form_to_the_cpu_device(ref):
    """a Crop whose flag the reference has no kernel for (its CPU device leaves the output as it is): not the device's"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = ch.Pyramid(74, DT_UINT8, (1, 8, 8, 10))
    c.conv(8, 3, 1); c.crop(None, dict(flag=2, axis=2), like_dims=[1, 8, 7, 9]); c.conv(8, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == ["Crop"], real


def test_golden_is_the_real_reference(ref):
    """tests/golden/crop_cases.npz (crop_helpers.write_golden) holds what the reference computes here, for every GPU case"""
    z = ch.golden()
    cases = ch.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    assert os.path.getsize(ch.GOLDEN) < 64 * 1024
    for case in sorted(stored):
        g, x = cases[case]()
        want = ch.reference_outputs(ref, g, x)
        assert ch.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not ch.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = ch.gpu_cases()
    q = lambda g, t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    for case, (x, like, p) in ch.SINGLE.items():        # input and output parameters differ in every single-node case
        g, _ = cases[case]()
        n = [n for n in g.nodes if n.op == "Crop"][0]
        assert q(g, n.inputs[0]) != q(g, n.outputs[0]), case
    g, _ = cases["chain_x2_identity_map"]()
    it = [n for n in g.nodes if n.op == "Interp"][0]
    assert q(g, it.inputs[0]) == q(g, it.outputs[0])
    g, _ = cases["chain_x2_off11"]()
    it = [n for n in g.nodes if n.op == "Interp"][0]
    assert q(g, it.inputs[0]) != q(g, it.outputs[0])
    g, _ = cases["chain_second_reader"]()
    it = [n for n in g.nodes if n.op == "Interp"][0]
    assert sum(it.outputs[0] in n.inputs for n in g.nodes) == 2
    for case in ch.TOPDOWN:
        g, x = cases[case]()
        assert (x == 0).any() and (x == 255).any(), case
        cr = [n for n in g.nodes if n.op == "Crop"][0]
        el = [n for n in g.nodes if n.op == "Eltwise"][0]
        assert cr.outputs[0] in el.inputs and (el.inputs[0] == cr.outputs[0]) == case.endswith(("first", "offset")), case
    assert len({ch.QSETS[k] for k in ch.QSETS}) == 3
    g, _ = cases["td_w19_c3_offset"]()
    assert g.tensors[0].dims == [1, 3, 15, 19] and 15 * 19 == 285
    g, _ = cases["td_batch2_ragged"]()
    total = int(np.prod(g.tensors[0].dims))
    assert total > 2 * 64 * 16 and total % (64 * 16) != 0 and total % 16 != 0
    g, _ = cases["ragged_blocks"]()
    out = int(np.prod(ch.SINGLE["ragged_blocks"][1]))
    assert out > 4 * 64 * 16 and out % (64 * 16) != 0
