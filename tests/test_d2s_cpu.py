"""Quantised DepthToSpace on the device, the parts that need no GPU: the tmfile writer and the library's reader, the support queries,
depthtospace_refusal's answers (each refusal by its name), shape inference, the committed golden against the numpy statement and
against the reference, and where the plugin's splitter puts the node."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import d2s_helpers as dh
import lut_helpers as lh
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3
G = dh.d2s_graph
X = (1, 8, 3, 5)

# (what is asked, type, input dims, block size, what else differs from a node that runs, the words of the refusal)
REFUSED = [
    ("rank_3", DT_UINT8, (8, 3, 5), 2, {}, "4-D tensors only"),
    ("rank_5", DT_INT8, (1, 8, 3, 5, 2), 2, {}, "4-D tensors only"),
    ("block_size_0", DT_UINT8, X, 0, dict(out_dims=[1, 8, 3, 5]), "block size must be at least 1"),
    ("block_size_negative", DT_INT8, X, -2, dict(out_dims=[1, 2, 6, 10]), "block size must be at least 1"),
    ("channels_not_divisible", DT_UINT8, (1, 6, 3, 5), 2, {}, "not a multiple of the block size squared"),
    ("channels_fewer_than_a_block", DT_INT8, (1, 3, 3, 5), 2, dict(out_dims=[1, 1, 6, 10]), "not a multiple of the block size squared"),
    ("constant_input", DT_UINT8, X, 2, dict(data_const=True), "must not be a constant"),
    ("per_channel_input", DT_INT8, X, 2, dict(in_quant=8), "per-tensor"),
    ("per_channel_output", DT_UINT8, X, 2, dict(out_quant=2), "per-tensor"),
    ("fp32", DT_FP32, X, 2, {}, "int8 and uint8 graphs only"),
]


def _error(g):
    return dh.library_outcome(tm2.write_tm2(g))[1]


def test_writer_and_library_reader_round_trip_operator_80():
    """fails without the feature: the library's reader does not know tm2 operator 80 and the file cannot be loaded"""
    assert tm2.OPTYPE["DepthToSpace"] == 80
    for r in (1, 2, 3, 7):
        g, _ = G(DT_UINT8, (1, 2 * r * r, 3, 5), r)
        b = tm2.write_tm2(g)
        node = [n for n in tm2.read_tm2(b).nodes if n.op == "DepthToSpace"]
        assert len(node) == 1 and node[0].params == {"block_size": r} and len(node[0].inputs) == 1
        L = capi.lib()
        h = L.tamd_graph_load_tm2(b, len(b))
        assert h, L.tamd_last_error()
        L.tamd_graph_destroy(h)
        # .. and the reader read THIS block size: the shape it infers follows it
        shape, err = dh.library_outcome(b)
        assert shape == (1, 2, 3 * r, 5 * r) and "depthtospace" not in err.lower(), (shape, err)
    g, _ = G(DT_INT8, X, 2)
    g.nodes[g.output_nodes[0]].params = {}               # the default is depthtospace.c's init_op: 1
    assert [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "DepthToSpace"][0].params == {"block_size": 1}


def test_models_builder_writes_the_node():
    b = models._B("sr", [1, 8, 4, 4])
    y = b.depth_to_space("ps", b.conv("up", b.cur, 12, 3, p=1), 2)
    assert b.dims(y) == [1, 3, 8, 8]
    assert b.g.nodes[-1].op == "DepthToSpace" and b.g.nodes[-1].params == {"block_size": 2}
    with pytest.raises(AssertionError):
        b.depth_to_space("bad", y, 2)                    # 3 channels: not a multiple of 4


def test_support_queries():
    L = capi.lib()
    A = dh.ask_d2s
    assert dh.OP_DEPTHTOSPACE == capi.OP_DEPTHTOSPACE == 34
    assert [L.tamd_op_supported(34, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 1, 1]
    assert [L.tamd_op_supported(33, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]
    assert [L.tamd_op_supported(35, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]
    for case, (dt, dims, r) in dh.SINGLE.items():       # what runs: every single-node case of the GPU tests
        assert A(I8 if dt == DT_INT8 else U8, dims, r) == 1, case
    for name, dt, dims, r, kw, _ in REFUSED:             # .. and what does not, each as the rule says
        code = {DT_INT8: I8, DT_FP32: F32}.get(dt, U8)
        assert A(code, dims, r, out_dims=kw.get("out_dims"), const_input=kw.get("data_const", False), in_quant=kw.get("in_quant"), out_quant=kw.get("out_quant")) == 0, name
    assert A(U8, X, 2, out_dims=[1, 2, 6, 11]) == 0 and A(I8, X, 2, out_dims=[2, 6, 10]) == 0 and A(U8, X, 2, out_dims=[1, 8, 3, 5]) == 0
    assert A(U8, X, 2, with_param=False) == 0
    assert A(U8, X, 2, inputs=2) == 0 and A(U8, X, 2, inputs=0) == 0
    assert A(FP16, X, 2) == 0


@pytest.mark.parametrize("case", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_forms_are_refused_by_name_when_a_file_carries_them(case):
    """through the tmfile reader and prerun's shape inference / validation, which run before the device is touched"""
    _, dt, dims, r, kw, words = case
    err = _error(G(dt, dims, r, **kw)[0])
    assert words in err, err


def test_a_node_that_runs_gets_as_far_as_the_device():
    for case, (dt, dims, r) in dh.SINGLE.items():
        assert "depthtospace" not in _error(G(dt, dims, r)[0]).lower(), case


# what depthtospace_refusal answers (tests/csrc/d2s_rules_check.cc): (input line, expected output line).  The line's fields: dtype
# has_param const in_quant out_quant block_size | rank and dims of the input | rank and dims of the output
VIEW = " view=%s order=0,1,4,2,5,3"
RULES = [
    ("u8 1 0 1 1 2 4 1 8 3 5", "OK r=2 out=1,2,6,10" + VIEW % "1,2,2,2,3,5"),
    ("i8 1 0 1 1 2 4 1 8 3 5", "OK r=2 out=1,2,6,10" + VIEW % "1,2,2,2,3,5"),
    ("u8 1 0 1 1 3 4 2 18 2 7", "OK r=3 out=2,2,6,21" + VIEW % "2,2,3,3,2,7"),
    ("u8 1 0 1 1 4 4 1 16 1 1", "OK r=4 out=1,1,4,4" + VIEW % "1,1,4,4,1,1"),
    ("i8 1 0 1 1 1 4 1 5 3 3", "OK r=1 out=1,5,3,3" + VIEW % "1,5,1,1,3,3"),                                         # a copy
    ("u8 1 0 1 1 2 4 1 8 3 5 4 1 2 6 10", "OK r=2 out=1,2,6,10" + VIEW % "1,2,2,2,3,5"),                             # the output's dims given, and right
    ("u8 1 0 1 1 2 4 1 8 3 5 4 1 2 6 11", "REFUSED DepthToSpace: the output does not have the dims the reference infers"),
    ("u8 1 0 1 1 2 4 1 8 3 5 3 2 6 10", "REFUSED DepthToSpace: the output does not have the dims the reference infers"),
    ("u8 0 0 1 1 2 4 1 8 3 5", "REFUSED DepthToSpace needs its parameter"),
    ("f32 1 0 1 1 2 4 1 8 3 5", "REFUSED DepthToSpace runs on the device in int8 and uint8 graphs only"),
    ("f16 1 0 1 1 2 4 1 8 3 5", "REFUSED DepthToSpace runs on the device in int8 and uint8 graphs only"),
    ("u8 1 0 1 1 2 3 8 3 5", "REFUSED DepthToSpace runs on the device on 4-D tensors only"),
    ("i8 1 0 1 1 2 5 1 8 3 5 2", "REFUSED DepthToSpace runs on the device on 4-D tensors only"),
    ("u8 1 0 1 1 2 0", "REFUSED DepthToSpace runs on the device on 4-D tensors only"),
    ("u8 1 0 1 1 0 4 1 8 3 5", "REFUSED DepthToSpace: the block size must be at least 1"),
    ("i8 1 0 1 1 -3 4 1 8 3 5", "REFUSED DepthToSpace: the block size must be at least 1"),
    ("u8 1 0 1 1 2 4 1 6 3 5", "REFUSED DepthToSpace: the channel count is not a multiple of the block size squared (the reference would drop channels)"),
    ("u8 1 0 1 1 3 4 1 8 3 5", "REFUSED DepthToSpace: the channel count is not a multiple of the block size squared (the reference would drop channels)"),
    ("u8 1 0 1 1 2147483647 4 1 8 3 5", "REFUSED DepthToSpace: the channel count is not a multiple of the block size squared (the reference would drop channels)"),      # no overflow on the way
    ("u8 1 0 1 1 46341 4 1 8 3 5", "REFUSED DepthToSpace: the channel count is not a multiple of the block size squared (the reference would drop channels)"),           # r * r leaves int
    ("u8 1 1 1 1 2 4 1 8 3 5", "REFUSED DepthToSpace: the input must not be a constant"),
    ("u8 1 0 8 1 2 4 1 8 3 5", "REFUSED DepthToSpace needs per-tensor quant params on both sides"),
    ("i8 1 0 1 2 2 4 1 8 3 5", "REFUSED DepthToSpace needs per-tensor quant params on both sides"),
    ("u8 1 0 0 1 2 4 1 8 3 5", "REFUSED DepthToSpace needs per-tensor quant params on both sides"),
    ("u8 1 0 1 1 2 4 1 8 0 5", "REFUSED DepthToSpace: every dimension must be at least 1"),
    ("u8 1 0 1 1 2 4 65536 32768 2 2", "REFUSED DepthToSpace: the tensor has more than 2^31 elements"),
    ("u8 1 0 1 1 2 4 1 4 2000000000 2000000000", "REFUSED DepthToSpace: the tensor has more than 2^31 elements"),
    ("u8 1 0 1 1 1 4 1 4 40000 40000", "REFUSED DepthToSpace: the tensor has more than 2^31 elements"),
    ("u8 1 0 1 1 2 4 1 4 1 536870000", "OK r=2 out=1,1,2,1073740000" + VIEW % "1,1,2,2,1,536870000"),                   # just below: 2147480000 elements
]


def test_depthtospace_refusal_names_every_refusal_and_resolves_the_shape(tmp_path):
    """the rule itself, as a stand-alone host program (its own main, host code only) under the address and undefined-behaviour sanitizers"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "d2s_rules_check")
    subprocess.check_call([hipcc, "-std=c++17", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "tengine_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "d2s_rules_check.cc"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], input="\n".join(r[0] for r in RULES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(RULES), out.stdout
    for (case, want), got in zip(RULES, lines):
        assert got == want, (case, got, want)
    assert len({w for _, w in RULES if w.startswith("REFUSED")}) >= 10           # every refusal has its own reason


SHAPES = [(k,) + v for k, v in dh.SINGLE.items()]


@pytest.mark.parametrize("case", SHAPES, ids=[s[0] for s in SHAPES])
def test_inferred_shape_is_the_numpy_statements(case):
    """a file whose output tensor carries NO useful shape: the library infers (N, C / r^2, H * r, W * r)"""
    name, dt, dims, r = case
    g, x = G(dt, dims, r)
    g.tensors[g.nodes[g.output_nodes[0]].outputs[0]].dims = [1, 1, 1, 1]
    shape, err = dh.library_outcome(tm2.write_tm2(g))
    assert shape == dh.numpy_d2s(x, r).shape == (dims[0], dims[1] // (r * r), dims[2] * r, dims[3] * r), (shape, err)
    assert "depthtospace" not in err.lower(), err


def test_golden_equals_the_numpy_statement_on_every_case():
    z = dh.golden()
    cases = dh.gpu_cases()
    assert {k[:-3] for k in z.files if k.endswith("__n")} == set(cases)
    assert os.path.getsize(dh.GOLDEN) < 64 * 1024
    for case, (dt, dims, r) in dh.SINGLE.items():
        g, x = cases[case][1]()
        assert np.array_equal(z[case + "__in"], x) and x.dtype == tm2.NP_OF_DT[dt], case
        assert int(z[case + "__n"]) == 1
        want = dh.numpy_d2s(x, r)
        assert z[case + "__out0"].dtype == want.dtype and np.array_equal(z[case + "__out0"], want), case
    # the graphs whose node reads the graph input: the node's part of the output is the statement too -- but for the byte -128 behind a
    # Concat of SEVERAL inputs, which the reference stores as 127 (concat_kernel_ref_int8.c), in place or copied
    for case, r, lead, planes in (("u8_concat_slice", 2, 3, 1), ("u8_concat_slice_odd_offset", 3, 1, 2)):
        x = z[case + "__in"]
        assert np.array_equal(z[case + "__out0"][:, lead:lead + planes], dh.numpy_d2s(x, r)), case
    for case in ("i8_into_concat_in_place", "i8_into_concat_copied"):
        x = z[case + "__in"]
        raw = dh.numpy_d2s(x, 2)
        assert (raw == -128).any(), case
        assert np.array_equal(z[case + "__out0"][:, :raw.shape[1]], np.where(raw == -128, 127, raw)), case


def test_cases_hold_what_they_are_named_for():
    cases = dh.gpu_cases()
    for case, (dt, dims, r) in dh.SINGLE.items():
        g, x = cases[case][1]()
        n = g.nodes[g.output_nodes[0]]
        q = lambda t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
        assert q(n.inputs[0]) != q(n.outputs[0]), case      # the parameters differ: the bytes are copied regardless
        raw = x.view(np.uint8)
        assert (raw == 0x80).any() and (raw == 0x7f).any() and (raw == 0).any() and (raw == 0xff).any(), case
        assert len(np.unique(raw)) == min(256, x.size), case
    assert (3 * 2) * (5 * 2) % 16 != 0 and 5 * 2 < 16                     # u8_rows_of_10: no chunk lies inside one row
    assert (24 * 2) % 16 == 0                                             # u8_aligned_rows_of_48: every chunk does
    for case, outc in (("i8_outc3_padding", 3), ("i8_outc16", 16), ("i8_outc20_batch2", 20), ("i8_r3", 4)):
        dt, dims, r = dh.SINGLE[case]
        assert dims[1] // (r * r) == outc
    g, _ = cases["i8_source_concat_slice"][1]()
    d = [n for n in g.nodes if n.op == "DepthToSpace"][0]
    cat = [n for n in g.nodes if n.op == "Concat"][0]
    assert d.inputs[0] == cat.inputs[1] and g.tensors[cat.inputs[0]].dims[1] == 16 and g.tensors[d.inputs[0]].dims[1] == 32
    for case in ("i8_into_concat_in_place", "i8_into_concat_copied", "u8_concat_slice", "u8_concat_slice_odd_offset"):
        g, _ = cases[case][1]()
        d = [n for n in g.nodes if n.op == "DepthToSpace"][0]
        cat = [n for n in g.nodes if n.op == "Concat"][0]
        assert d.outputs[0] in cat.inputs and len(cat.inputs) >= 2, case
        if case.startswith("u8"):
            i = cat.inputs.index(d.outputs[0])
            assert 0 < i < len(cat.inputs) - 1, case                      # neighbours on both sides
    g, _ = cases["u8_concat_slice_odd_offset"][1]()
    assert g.tensors[[n for n in g.nodes if n.op == "Concat"][0].inputs[0]].dims == [1, 1, 3, 3]      # the node's planes start at byte 9


@pytest.mark.parametrize("case", sorted(dh.gpu_cases()))
def test_golden_is_the_real_reference(ref, case):
    """tests/golden/d2s_cases.npz (tools/make_golden_d2s.py) holds what the reference computes here"""
    z = dh.golden()
    dt, build = dh.gpu_cases()[case]
    g, x = build()
    assert np.array_equal(z[case + "__in"], x)
    want = dh.reference_outputs(ref, g, x, dt)
    assert dh.equals_golden(z, case, want), case
    want[0].reshape(-1)[0] ^= 1                          # .. and the comparison is one: a single changed bit is seen
    assert not dh.equals_golden(z, case, want), case


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("build", [dh.espcn_tail, dh.edsr_upsampler], ids=["espcn_tail", "edsr_upsampler"])
def test_plugin_keeps_sub_pixel_convolution_in_one_hip_subgraph(ref, build, dtype):
    """fails without the feature: the plugin's operator table does not know the node and the split gives HIP / CPU (/ HIP)"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = build(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and {dh.REF_OP_NAME, "Convolution"} <= set(real[0][1]), real


@pytest.mark.parametrize("build", [dh.espcn_tail, dh.edsr_upsampler], ids=["espcn_tail", "edsr_upsampler"])
def test_plugin_leaves_the_node_of_an_fp32_graph_to_the_cpu_device(ref, build):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = build(DT_FP32)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    nodes = [(dev, ops) for dev, ops in real if dh.REF_OP_NAME in ops]
    assert len(nodes) == 1 and nodes[0][0] != "HIP", real
    assert real[0][0] == "HIP" and "Convolution" in real[0][1], real
    assert len(real) == (2 if build is dh.espcn_tail else 3), real


def test_plugin_leaves_a_refused_form_to_the_cpu_device(ref):
    """C not divisible by r^2 (the reference's CPU device drops the channels behind outc * r^2): not the device's"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = dh.SubPixel(86, DT_UINT8, (1, 8, 4, 4))
    c.conv(9, 3, 1)
    x9 = c.cur
    y = c._var("odd", [1, 2, 8, 8], c.quant(x9))
    c.last = c.g.add_node("odd", "DepthToSpace", [x9], [y], block_size=2)
    c.cur = y
    c.conv(4, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == [dh.REF_OP_NAME], real
