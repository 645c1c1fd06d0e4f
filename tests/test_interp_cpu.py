"""Quantised nearest Interp on the device, the parts that need no GPU: the tmfile writer and reader, shape inference against the real
reference library, the byte map on all 256 bytes and the index vectors against what the reference computes, what the support queries
answer, where the plugin's splitter puts the node, the committed golden against the reference, and the two host builders alone under the
address / undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (id, type, (in scale, in zp), (out scale, out zp)): what each set is for is in its id
TABLE_SETS = [
    ("i8_scales_differ", DT_INT8, (0.05, 0), (0.031, 0)),
    ("i8_equal_scales", DT_INT8, (0.05, 0), (0.05, 0)),
    ("u8_zp0", DT_UINT8, (0.05, 0), (0.031, 12)),
    ("u8_zp77", DT_UINT8, (0.05, 77), (0.031, 12)),
    ("u8_zp255", DT_UINT8, (0.05, 255), (0.04, 200)),
    ("u8_equal", DT_UINT8, (0.05, 77), (0.05, 77)),
    ("i8_saturates_both_ends", DT_INT8, (0.2, 0), (0.05, 0)),
    ("u8_saturates_both_ends", DT_UINT8, (0.2, 128), (0.05, 128)),
]
# (in, out, parameter along that axis): the index cases; all stay inside the input
INDEX_CASES = [(3, 6, 2.0), (4, 6, 1.5), (7, 10, 1.5), (8, 4, 0.5), (5, 3, 0.6), (5, 7, None), (13, 26, 2.0)]


def _table(case):
    _, dtype, in_q, out_q = case
    return capi.interp_table(dtype, lh.f32(in_q[0]), in_q[1], lh.f32(out_q[0]), out_q[1])


def _written_cases():
    return [(k, dtype, dims, p) for dtype in (DT_INT8, DT_UINT8) for k, (dims, p) in ih.GEOMETRY.items()]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8])
def test_writer_and_reader_round_trip_the_five_parameters(dtype):
    p = {"resize_type": 1, "width_scale": lh.f32(1.5), "height_scale": lh.f32(0.6), "output_width": 11, "output_height": 7}
    g = ih.unary_graph(dtype, (1, 16, 7, 4), (0.05, 0), (0.031, 0), p)
    back = tm2.read_tm2(tm2.write_tm2(g))
    node = [n for n in back.nodes if n.op == "Interp"]
    assert len(node) == 1 and node[0].params == p


@pytest.mark.parametrize("case", _written_cases(), ids=lambda c: "%s-%d" % (c[0], c[1]))
def test_written_tmfile_runs_in_the_reference_and_the_inferred_shapes_agree(ref, case):
    """the reference loads the file and runs it; the shape IT infers is the one the library infers (the sizes-only case included) and
    the one the test wrote"""
    _, dtype, dims, p = case
    g, x = ih.single(dtype, dims, p, 5)
    b = tm2.write_tm2(g)
    out = ref.run_model(b, x, lh.ref_mode(ref, dtype))
    assert len(out) == 1 and out[0].dtype == lh.NP[dtype]
    shape, err = ih.library_output_shape(capi, b)
    assert shape == out[0].shape == tuple(dims[:2]) + ih.out_hw(dims[2], dims[3], p), (shape, out[0].shape, err)


def test_unstable_sizes_only_node_is_refused_by_name():
    """11 -> 13: the scale 13 / 11 gives 12 when the reference infers again; the library says so instead of planning either size"""
    g, _ = ih.single(DT_INT8, (1, 8, 11, 11), ih.by_size(13, 13), 5)
    _, err = ih.library_output_shape(capi, tm2.write_tm2(g))
    assert "does not keep this output size" in err, err


@pytest.mark.parametrize("case", TABLE_SETS, ids=[s[0] for s in TABLE_SETS])
def test_table_is_the_reference_on_every_byte(ref, case):
    """a 1x Interp over a tensor that holds all 256 byte values, in the reference, against tamd_interp_table: byte equality"""
    _, dtype, in_q, out_q = case
    b = tm2.write_tm2(ih.unary_graph(dtype, (1, 16, 4, 4), in_q, out_q, ih.by_scale(1.0)))
    want = ref.run_model(b, lh.all_bytes(dtype), lh.ref_mode(ref, dtype))[0]
    got = _table(case)
    assert got is not None and got.shape == (256,)
    assert np.array_equal(got, want.reshape(-1).view(np.uint8)), np.nonzero(got != want.reshape(-1).view(np.uint8))[0]


def test_parameter_sets_reach_the_branches_they_are_named_for():
    sets = {s[0]: s for s in TABLE_SETS}
    ident = np.arange(256, dtype=np.uint8)
    eq = _table(sets["i8_equal_scales"])
    assert eq[0x80] == 0x81                                             # -128 comes out as -127: an int8 "copy" would be wrong
    assert np.array_equal(np.delete(eq, 0x80), np.delete(ident, 0x80))
    assert np.array_equal(_table(sets["u8_equal"]), ident)
    for zp in (0, 12, 77, 128, 255):
        assert np.array_equal(capi.interp_table(DT_UINT8, lh.f32(0.05), zp, lh.f32(0.05), zp), ident), zp
    i8 = _table(sets["i8_saturates_both_ends"]).view(np.int8)
    assert (i8 == 127).sum() > 1 and (i8 == -127).sum() > 1 and i8.min() == -127
    u8 = _table(sets["u8_saturates_both_ends"])
    assert (u8 == 255).sum() > 1 and (u8 == 0).sum() > 1
    assert _table(sets["i8_scales_differ"]).view(np.int8).min() == -127 and _table(sets["i8_scales_differ"])[0] == 0
    assert _table(sets["u8_zp0"])[0] == 12                              # byte 0 does not map to 0 wherever a zero point is in play
    assert _table(sets["u8_zp77"])[77] == 12 and _table(sets["u8_zp255"])[255] == 200
    assert capi.interp_table(DT_FP32, 0.05, 0, 0.02, 0) is None


@pytest.mark.parametrize("case", INDEX_CASES, ids=lambda c: "%d-%d" % (c[0], c[1]))
def test_indices_are_the_reference(ref, case):
    """a uint8 image whose pixels are all distinct under the identity byte map: the reference's output names the source pixel of every
    output pixel, rows and columns (the same case on both axes: H * W <= 256)"""
    n_in, n_out, s = case
    p = ih.by_size(n_out, n_out) if s is None else ih.by_scale(s)
    assert ih.out_hw(n_in, n_in, p) == (n_out, n_out)
    x = np.arange(n_in * n_in, dtype=np.uint8).reshape(1, 1, n_in, n_in)
    out = ref.run_model(tm2.write_tm2(ih.unary_graph(DT_UINT8, x.shape, (0.05, 77), (0.05, 77), p)), x, ref.MODE_UINT8)[0]
    assert out.shape == (1, 1, n_out, n_out)
    scale = lh.f32(s) if s is not None else float(np.float32(n_out) / np.float32(n_in))
    idx = capi.interp_indices(n_in, n_out, scale)
    assert idx is not None and idx.max() < n_in
    src = out[0, 0].astype(np.int64)
    assert np.array_equal(src // n_in, np.repeat(idx[:, None], n_out, 1)) and np.array_equal(src % n_in, np.repeat(idx[None, :], n_out, 0))


def test_indices_refuse_what_leaves_the_input():
    assert capi.interp_indices(4, 4, 0.5) is None and capi.interp_indices(4, 0, 1.0) is None and capi.interp_indices(4, 4, 0.0) is None
    assert list(capi.interp_indices(4, 8, 2.0)) == [0, 0, 1, 1, 2, 2, 3, 3]


def test_support_queries():
    L = capi.lib()
    F32, FP16, I8, U8 = 0, 1, 2, 3
    assert [L.tamd_op_supported(ih.OP_INTERP, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 1, 1]
    x2, dims = ih.by_scale(2.0), [1, 16, 4, 4]
    assert ih.ask_node(capi, I8, dims, x2) == 1 and ih.ask_node(capi, U8, dims, x2) == 1
    assert ih.ask_node(capi, I8, [2, 17, 5, 3], ih.by_scale(2.0, 3.0)) == 1                 # any batch, per-axis scales
    assert ih.ask_node(capi, U8, [1, 16, 7, 4], ih.by_scale(1.5)) == 1 and ih.ask_node(capi, I8, [1, 16, 8, 8], ih.by_scale(0.5)) == 1
    assert ih.ask_node(capi, I8, [1, 8, 5, 5], ih.by_size(7, 7)) == 1
    assert ih.ask_node(capi, F32, dims, x2) == 0
    assert ih.ask_node(capi, I8, dims, ih.by_scale(2.0, resize_type=2)) == 0 and ih.ask_node(capi, U8, dims, ih.by_scale(2.0, resize_type=4)) == 0
    assert ih.ask_node(capi, I8, [16, 4, 4], x2) == 0
    assert ih.ask_node(capi, I8, dims, x2, const_input=True) == 0
    assert ih.ask_node(capi, I8, [1, 8, 11, 11], ih.by_size(13, 13)) == 0                   # 11 -> 13 infers to 12 the second time
    assert ih.ask_node(capi, I8, [1, 8, 11, 11], ih.by_size(13, 13), out_dims=[1, 8, 12, 12]) == 0
    # .. and as the plugin sees that node after the reference's first inference: scales filled in, the tensor still 13 x 13
    filled = dict(ih.by_size(13, 13), width_scale=float(np.float32(13) / np.float32(11)), height_scale=float(np.float32(13) / np.float32(11)))
    assert ih.ask_node(capi, I8, [1, 8, 11, 11], filled, out_dims=[1, 8, 13, 13]) == 0
    assert ih.ask_node(capi, I8, dims, x2, out_dims=[1, 16, 8, 9]) == 0
    # the operators that were there keep their answers and their codes
    assert [L.tamd_op_supported(op, I8) for op in range(20)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert L.tamd_op_supported(21, I8) == 0


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8])
def test_plugin_keeps_the_neck_in_one_hip_subgraph(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ih.neck_graph(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and "Interp" in real[0][1], real


def test_plugin_leaves_the_fp32_neck_interp_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ih.neck_graph(DT_FP32)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    on_hip = {o for dev, os_ in real if dev == "HIP" for o in os_}
    on_cpu = {o for dev, os_ in real if dev != "HIP" for o in os_}
    # Sigmoid was an fp32 CPU node before (tests/test_lut_cpu.py); the Eltwise wedged between it and the Interp goes where they go
    assert "Interp" in on_cpu and on_cpu <= {"Interp", "Sigmoid", "Eltwise"} and "Interp" not in on_hip and {"Convolution", "Pooling", "Concat"} <= on_hip, real


def test_bilinear_interp_stays_a_cpu_node_between_two_device_subgraphs(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ih.bilinear_graph()
    real = _real(tp._split_only(ref, g, x, ref.MODE_INT8))
    assert [(dev == "HIP", ops) for dev, ops in real] == [(True, ["Convolution"]), (False, ["Interp"]), (True, ["Convolution"])], real


def test_golden_is_the_real_reference(ref):
    """tests/golden/interp_nearest_cases.npz (tools/make_golden_interp.py) holds what the reference computes here, for every GPU case"""
    z = ih.golden()
    cases = ih.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    for case in sorted(stored):
        dtype, build = cases[case]
        g, x = build()
        want = ih.reference_outputs(ref, g, x, dtype)
        assert ih.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not ih.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    """the -128 case holds -128, the identity case has equal quantisation, the in-place concat case starts the Interp's planes at an odd byte"""
    g, x = ih.gpu_cases()["i8_one_vector_minus128"][1]()
    assert (x == -128).sum() >= 2
    g, _ = ih.gpu_cases()["u8_concat_in_place_odd_start"][1]()
    cat = [n for n in g.nodes if n.op == "Concat"][0]
    lead = g.tensors[cat.inputs[0]].dims
    assert (lead[1] * lead[2] * lead[3]) % 2 == 1
    assert [n.op for n in g.nodes if cat.inputs[1] in n.outputs] == ["Interp"]
    for t in cat.inputs:
        assert (g.tensors[t].scales, g.tensors[t].zero_points) == (g.tensors[cat.outputs[0]].scales, g.tensors[cat.outputs[0]].zero_points)
    g, _ = ih.gpu_cases()["u8_identity"][1]()
    assert capi.interp_table(DT_UINT8, g.tensors[0].scales[0], g.tensors[0].zero_points[0], g.tensors[1].scales[0], g.tensors[1].zero_points[0]).tolist() == list(range(256))


def test_builders_alone_under_the_sanitizers(tmp_path):
    """tests/csrc/interp_tables_check.cc + csrc/interp_tables.cc and nothing else, built with -fsanitize=address,undefined and run as a
    child process: every table and index vector is built, the degenerate inputs are refused, the program exits 0, and its answers are
    the library's (another compiler, the same bytes)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "interp_tables_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "interp_tables_check.cc"), os.path.join(ROOT, "tengine_amd", "csrc", "interp_tables.cc"),
                           "-lm", "-o", exe])
    hexf = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]
    args, want = [], []
    for case in TABLE_SETS:
        _, dtype, in_q, out_q = case
        args += ["t", str(dtype), hexf(in_q[0]), str(in_q[1]), hexf(out_q[0]), str(out_q[1])]
        want.append(_table(case).tobytes().hex())
    for n_in, n_out, s in INDEX_CASES + [(4, 4, 0.5)]:
        scale = lh.f32(s) if s is not None else float(np.float32(n_out) / np.float32(n_in))
        args += ["i", str(n_in), str(n_out), hexf(scale)]
        idx = capi.interp_indices(n_in, n_out, scale)
        want.append("refused" if idx is None else ",".join(str(v) for v in idx))
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == want
