"""Quantised Split and ShuffleChannel on the device, the parts that need no GPU: the tmfile writer and reader, shape inference against
the real reference library, the ShuffleChannel source vector and the uint8 Split byte map (all 256 bytes) against what the reference
computes, what the support queries answer, where the plugin's splitter puts the nodes, the committed golden against the reference, and
the two host builders alone under the address / undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lut_helpers as lh
import shuffle_helpers as sh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3

# (id, (in scale, in zp), (out scale, out zp)) of the uint8 Split byte map: what each set is for is in its id
TABLE_SETS = [
    ("equal", (0.05, 77), (0.05, 77)),
    ("zp0_to_zp255", (0.05, 0), (0.05, 255)),
    ("zp255_to_zp0", (0.04, 255), (0.05, 0)),
    ("rescale_above_1", (0.05, 77), (0.031, 12)),
    ("rescale_below_1", (0.031, 12), (0.05, 77)),
    ("saturates_both_ends", (0.2, 128), (0.05, 128)),
    ("ties", (0.05, 3), (0.1, 4)),                        # rescale 0.5: every odd difference lands on a tie
    ("awkward_ratio", (0.0173, 101), (0.0291, 37)),
]
SHUFFLE_SETS = [(12, 3), (20, 2), (116, 2), (24, 4), (8, 1), (8, 8), (6, 2)]


def _table(case):
    _, in_q, out_q = case
    return capi.split_table(lh.f32(in_q[0]), in_q[1], lh.f32(out_q[0]), out_q[1])


def test_writer_and_reader_round_trip_both_parameter_blobs():
    g, _ = sh.split_graph(DT_INT8, (1, 12, 3, 5), [5, 7])
    back = tm2.read_tm2(tm2.write_tm2(g))
    node = [n for n in back.nodes if n.op == "Split"]
    assert len(node) == 1 and node[0].params == {"axis": 1, "split_dim": 1, "is_caffe": 0, "is_onnx": 1, "split_sizes": [5, 7]}
    assert len(node[0].outputs) == 2
    g, _ = sh.caffe_split_graph()
    node = [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "Split"]
    assert node[0].params["is_caffe"] == 1 and node[0].params["split_sizes"] == []
    g, _ = sh.shuffle_graph(DT_UINT8, (1, 12, 3, 5), 3)
    node = [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "ShuffleChannel"]
    assert len(node) == 1 and node[0].params == {"group": 3}


WRITTEN = ["i8_shuffle_cross_vector_batch2", "u8_shuffle_batch2", "i8_split_unaligned", "i8_split_one_aligned_batch2", "u8_split_requant_and_identity",
           "i8_unit_half6", "i8_unit_half58_b2", "u8_unit_half6", "i8_down_half10"]


@pytest.mark.parametrize("case", WRITTEN)
def test_written_tmfile_runs_in_the_reference_and_the_inferred_shapes_agree(ref, case):
    """the reference loads the file and runs it, at batch 2 as well; the shape IT infers is the one the library infers"""
    dtype, build = sh.gpu_cases()[case]
    g, x = build()
    b = tm2.write_tm2(g)
    out = ref.run_model(b, x, lh.ref_mode(ref, dtype))
    assert len(out) == 1 and out[0].dtype == lh.NP[dtype]
    shape, err = sh.library_outcome(b)
    assert shape == out[0].shape, (shape, out[0].shape, err)
    assert "not supported" not in err and "split" not in err.lower() and "shuffle" not in err.lower(), err


def test_reference_semantics_are_the_ones_the_device_is_built_on(ref):
    """int8 Split is x[:, a:b] byte for byte, also when its scale differs (seen through a one-output Split); ShuffleChannel is the
    reshape / transpose in both types at batch 2; the reference's Concat of several inputs turns -128 into 127 between equal scales"""
    for dtype in (DT_INT8, DT_UINT8):
        g, x = sh.shuffle_graph(dtype, (2, 20, 3, 2), 2, out_q=(0.031, 5 if dtype == DT_UINT8 else 0), force=-128 if dtype == DT_INT8 else None)
        out = ref.run_model(tm2.write_tm2(g), x, lh.ref_mode(ref, dtype))[0]
        assert np.array_equal(out, x.reshape(2, 2, 10, 3, 2).transpose(0, 2, 1, 3, 4).reshape(x.shape))
    g, x = sh.split_graph(DT_INT8, (2, 12, 3, 5), [5, 7], out_qs=[(0.031, 0), (0.02, 0)], force=-128)
    g.output_nodes = [len(g.nodes) - 2]                  # the Split itself: its output 0 is what the reference shows
    out = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8)[0]
    assert (x[:, :5] == -128).sum() >= 1 and np.array_equal(out, x[:, :5])
    g, x = sh.split_graph(DT_INT8, (1, 12, 3, 5), [5, 7], force=-128)
    out = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8)[0]
    want = np.concatenate([x[:, 5:], x[:, :5]], 1)
    assert (want == -128).sum() >= 2 and np.array_equal(out, np.where(want == -128, 127, want))


@pytest.mark.parametrize("case", SHUFFLE_SETS, ids=lambda c: "%d-%d" % c)
def test_shuffle_sources_are_the_reference(ref, case):
    """a uint8 tensor whose channels hold distinct values: the reference's output names the source channel of every output channel"""
    channels, group = case
    x = np.repeat(np.arange(channels, dtype=np.uint8), 6).reshape(1, channels, 2, 3)
    g, _ = sh.shuffle_graph(DT_UINT8, x.shape, group)
    out = ref.run_model(tm2.write_tm2(g), x, ref.MODE_UINT8)[0]
    src = capi.shuffle_sources(channels, group)
    assert src is not None and sorted(src) == list(range(channels))
    assert np.array_equal(out, x[:, src])
    assert np.array_equal(src, np.arange(channels).reshape(group, channels // group).T.reshape(-1))


def test_shuffle_sources_refuse_what_the_reference_does_not_write():
    assert capi.shuffle_sources(12, 5) is None and capi.shuffle_sources(12, 0) is None and capi.shuffle_sources(12, -2) is None
    assert capi.shuffle_sources(0, 1) is None
    assert list(capi.shuffle_sources(6, 2)) == [0, 3, 1, 4, 2, 5]


@pytest.mark.parametrize("case", TABLE_SETS, ids=[s[0] for s in TABLE_SETS])
def test_split_table_is_the_reference_on_every_byte(ref, case):
    """a one-output uint8 Split over a tensor that holds all 256 byte values, in the reference, against tamd_split_table: byte equality.
    This is what guards the fused multiply-add in csrc/chanmap_tables.cc"""
    _, in_q, out_q = case
    g, _ = sh.split_graph(DT_UINT8, (1, 16, 4, 4), [16], in_q=in_q, out_qs=[out_q])
    g.output_nodes = [len(g.nodes) - 2]                  # the Split itself
    want = ref.run_model(tm2.write_tm2(g), lh.all_bytes(DT_UINT8), ref.MODE_UINT8)[0]
    got = _table(case)
    assert got is not None and got.shape == (256,)
    assert np.array_equal(got, want.reshape(-1)), np.nonzero(got != want.reshape(-1))[0]


def test_parameter_sets_reach_the_branches_they_are_named_for():
    sets = {s[0]: s for s in TABLE_SETS}
    ident = np.arange(256, dtype=np.uint8)
    assert np.array_equal(_table(sets["equal"]), ident)
    for zp in (0, 12, 77, 128, 255):
        assert np.array_equal(capi.split_table(lh.f32(0.05), zp, lh.f32(0.05), zp), ident), zp
    assert _table(sets["zp0_to_zp255"])[0] == 255 and (_table(sets["zp0_to_zp255"]) == 255).all()
    assert _table(sets["zp255_to_zp0"])[255] == 0 and (_table(sets["zp255_to_zp0"]) == 0).all()
    u8 = _table(sets["saturates_both_ends"])
    assert (u8 == 255).sum() > 1 and (u8 == 0).sum() > 1
    assert lh.f32(0.05) / lh.f32(0.031) > 1 > lh.f32(0.031) / lh.f32(0.05)
    assert _table(sets["rescale_above_1"])[77] == 12 and _table(sets["rescale_below_1"])[12] == 77
    assert list(_table(sets["ties"])[:8]) == [3, 3, 4, 4, 5, 5, 6, 6]        # (b - 3) * 0.5 + 4; roundf: ties away from zero, 2.5 -> 3


def _split_error(g):
    return sh.library_outcome(tm2.write_tm2(g))[1]


def test_support_queries():
    L = capi.lib()
    for op in (sh.OP_SPLIT, sh.OP_SHUFFLECHANNEL):
        assert [L.tamd_op_supported(op, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 1, 1]
    # Split: what runs
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7]) == 1 and sh.ask_split(U8, [1, 12, 3, 5], [5, 7]) == 1
    assert sh.ask_split(I8, [2, 32, 3, 2], [16, 8, 8]) == 1 and sh.ask_split(I8, [1, 16, 4, 4], [16]) == 1
    assert sh.ask_split(I8, [1, 8, 2, 2], [1] * 8) == 1
    # .. and what does not, each for its own reason
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7], num=-1) == 0                             # is_caffe
    assert sh.ask_split(I8, [1, 12, 3, 5], [], num=0, out_dims=[[1, 12, 3, 5]] * 2) == 0    # no split_sizes
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 6]) == 0                                     # sum != C
    assert sh.ask_split(I8, [1, 12, 3, 5], [12, 0], out_dims=[[1, 12, 3, 5], [1, 0, 3, 5]]) == 0
    assert sh.ask_split(I8, [4, 12, 3, 5], [1, 3], axis=0, out_dims=[[1, 12, 3, 5], [3, 12, 3, 5]]) == 0
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7], axis=-3) == 0 and sh.ask_split(I8, [1, 12, 3, 5], [1, 2], axis=2, out_dims=[[1, 12, 1, 5], [1, 12, 2, 5]]) == 0
    assert sh.ask_split(I8, [12, 3, 5], [5, 7], out_dims=[[5, 3, 5], [7, 3, 5]]) == 0        # 3-D
    assert sh.ask_split(U8, [2, 12, 3, 5], [5, 7]) == 0 and sh.ask_split(I8, [2, 12, 3, 5], [5, 7]) == 1      # uint8 at batch 2
    assert sh.ask_split(F32, [1, 12, 3, 5], [5, 7]) == 0
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7], const_input=True) == 0
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7], out_dims=[[1, 5, 3, 5]]) == 0            # one size per output
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7], out_dims=[[1, 5, 3, 5], [1, 7, 3, 4]]) == 0
    assert sh.ask_split(I8, [1, 18, 2, 2], [2] * 9) == 0                                    # more than TAMD_SPLIT_MAX
    assert sh.ask_split(I8, [1, 12, 3, 5], [5, 7], out_quant=12) == 0                       # per-channel quantisation
    # ShuffleChannel
    assert sh.ask_shuffle(I8, [1, 12, 3, 5], 3) == 1 and sh.ask_shuffle(U8, [2, 12, 3, 5], 3) == 1 and sh.ask_shuffle(I8, [2, 20, 3, 2], 2) == 1
    assert sh.ask_shuffle(I8, [1, 8, 3, 3], 1) == 1 and sh.ask_shuffle(I8, [1, 8, 3, 3], 8) == 1
    assert sh.ask_shuffle(I8, [1, 12, 3, 5], 5) == 0 and sh.ask_shuffle(U8, [1, 12, 3, 5], 0) == 0         # C % group != 0
    assert sh.ask_shuffle(F32, [1, 12, 3, 5], 3) == 0
    assert sh.ask_shuffle(I8, [12, 3, 5], 3) == 0 and sh.ask_shuffle(I8, [1, 12, 3, 5], 3, const_input=True) == 0
    assert sh.ask_shuffle(I8, [1, 12, 3, 5], 3, with_param=False) == 0
    # the operators that were there keep their answers and their codes; 21 stays a reserved, never-supported value
    assert [L.tamd_op_supported(op, I8) for op in range(21)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1]
    assert [L.tamd_op_supported(op, U8) for op in range(21)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    assert [L.tamd_op_supported(op, F32) for op in range(21)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0]
    assert [L.tamd_op_supported(21, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0] and L.tamd_op_supported(24, I8) == 0


def test_refused_forms_are_refused_by_name_when_a_file_carries_them():
    """through the tmfile reader and prerun's validation (which run before the device is touched): the form, not a shape mismatch"""
    assert "is_caffe" in _split_error(sh.caffe_split_graph()[0])
    g, _ = sh.split_graph(DT_INT8, (1, 12, 3, 5), [5, 7])
    [n for n in g.nodes if n.op == "Split"][0].params["split_sizes"] = []
    assert "without split_sizes" in _split_error(g)
    g, _ = sh.split_graph(DT_INT8, (1, 12, 3, 5), [5, 6])
    assert "do not add up" in _split_error(g)
    g, _ = sh.split_graph(DT_INT8, (1, 12, 3, 5), [5, 7], is_onnx=0)       # the reference's loader then leaves the axis at 0
    assert "axis 1" in _split_error(g)
    g, _ = sh.split_graph(DT_UINT8, (2, 12, 3, 5), [5, 7])
    assert "batch 1" in _split_error(g)
    g, _ = sh.shuffle_graph(DT_INT8, (1, 12, 3, 5), 5)
    assert "must divide" in sh.library_outcome(tm2.write_tm2(g))[1]
    g, _ = sh.shuffle_graph(DT_FP32, (1, 12, 3, 5), 3)
    assert "int8 and uint8 graphs only" in sh.library_outcome(tm2.write_tm2(g))[1]


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8])
def test_plugin_keeps_the_unit_in_one_hip_subgraph(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = sh.basic_unit_graph(dtype, 6)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and {"Split", "ShuffleChannel", "Concat", "Convolution"} <= set(real[0][1]), real


def test_plugin_leaves_both_operators_of_the_fp32_unit_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = sh.basic_unit_graph(DT_FP32, 6)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    on_hip = {o for dev, os_ in real if dev == "HIP" for o in os_}
    on_cpu = {o for dev, os_ in real if dev != "HIP" for o in os_}
    assert {"Split", "ShuffleChannel"} <= on_cpu and not ({"Split", "ShuffleChannel"} & on_hip) and "Convolution" in on_hip, real


def test_caffe_split_stays_a_cpu_node_between_device_subgraphs(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = sh.caffe_split_graph()
    real = _real(tp._split_only(ref, g, x, ref.MODE_INT8))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == ["Split"], real
    assert real[0][1] == ["Convolution"] and "Concat" in real[2][1], real


def test_golden_is_the_real_reference(ref):
    """tests/golden/shuffle_cases.npz (tools/make_golden_shuffle.py) holds what the reference computes here, for every GPU case"""
    z = sh.golden()
    cases = sh.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    assert os.path.getsize(sh.GOLDEN) < 64 * 1024
    for case in sorted(stored):
        dtype, build = cases[case]
        g, x = build()
        want = sh.reference_outputs(ref, g, x, dtype)
        assert sh.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not sh.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = sh.gpu_cases()
    for k in ("i8_shuffle_one_vector_minus128", "i8_split_scale_differs_minus128", "i8_split_cat_shuffle_minus128"):
        g, x = cases[k][1]()
        assert (x == -128).sum() >= 2, k
    g, _ = cases["i8_shuffle_one_vector_minus128"][1]()
    assert g.tensors[0].scales != g.tensors[1].scales
    g, _ = cases["i8_split_scale_differs_minus128"][1]()
    sp = [n for n in g.nodes if n.op == "Split"][0]
    assert all(g.tensors[t].scales != g.tensors[sp.inputs[0]].scales for t in sp.outputs)
    g, _ = cases["u8_split_requant_and_identity"][1]()
    sp = [n for n in g.nodes if n.op == "Split"][0]
    q = lambda t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    tabs = [capi.split_table(*q(sp.inputs[0]), *q(t)).tolist() for t in sp.outputs]
    assert tabs[0] != list(range(256)) and tabs[1] == list(range(256))
    for k in sh.UNITS:                                   # every Concat in front of a ShuffleChannel carries its inputs' quantisation
        g, _ = cases["i8_" + k][1]()
        for n in g.nodes:
            if n.op == "Concat":
                assert all(g.tensors[t].scales == g.tensors[n.outputs[0]].scales for t in n.inputs), k


def test_builders_alone_under_the_sanitizers(tmp_path):
    """tests/csrc/chanmap_tables_check.cc + csrc/chanmap_tables.cc and nothing else, built with -fsanitize=address,undefined and run as
    a child process: every table and source vector is built, the degenerate inputs are refused, the program exits 0, and its answers
    are the library's (another compiler, the same bytes)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "chanmap_tables_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "chanmap_tables_check.cc"), os.path.join(ROOT, "tengine_amd", "csrc", "chanmap_tables.cc"),
                           "-lm", "-o", exe])
    hexf = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]
    args, want = [], []
    for case in TABLE_SETS:
        _, in_q, out_q = case
        args += ["t", hexf(in_q[0]), str(in_q[1]), hexf(out_q[0]), str(out_q[1])]
        want.append(_table(case).tobytes().hex())
    for channels, group in SHUFFLE_SETS + [(12, 5)]:
        args += ["s", str(channels), str(group)]
        src = capi.shuffle_sources(channels, group)
        want.append("refused" if src is None else ",".join(str(v) for v in src))
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == want
