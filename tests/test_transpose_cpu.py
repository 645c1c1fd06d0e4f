"""Quantised Transpose on the device, the parts that need no GPU: the byte map (all 256 bytes, both types) against what the reference
computes, the identity order as the pure map, every refusal by its name, the canonical geometry, the support queries, the tmfile writer
and reader, where the plugin's splitter puts the node, and the committed golden against the reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lut_helpers as lh
import transpose_helpers as th
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3
T = th.transpose_graph
TABLES = [(dt, s) for dt in (DT_UINT8, DT_INT8) for s in th.TABLE_SETS[dt]]
TABLE_IDS = ["%s_%s" % ("i8" if dt == DT_INT8 else "u8", s[0]) for dt, s in TABLES]


@pytest.mark.parametrize("dtype,case", TABLES, ids=TABLE_IDS)
def test_transpose_table_is_the_golden_on_every_byte(dtype, case):
    """tamd_transpose_table against the bytes the reference made of the raw bytes 0 .. 255 (a (1, 2, 16, 16) tensor through a Transpose),
    as the golden holds them"""
    got = th.table_of(dtype, case[1], case[2])
    assert got is not None and got.shape == (256,) and got.dtype == lh.NP[dtype]
    want = th.golden()[th.table_key(dtype, case[0])]
    assert want.dtype == got.dtype and np.array_equal(got, want), np.nonzero(got != want)[0]


@pytest.mark.parametrize("dtype,case", TABLES, ids=TABLE_IDS)
def test_transpose_table_is_the_reference_on_every_byte(ref, dtype, case):
    """.. and against the reference itself, where it is built"""
    g, x = th.table_case(dtype, case[1], case[2])
    assert np.array_equal(x[0, 1].reshape(-1).view(np.uint8), np.arange(256))
    want = th.reference_outputs(ref, g, x, dtype)[0]
    assert want.shape == (1, 2, 16, 16)
    assert np.array_equal(th.table_of(dtype, case[1], case[2]), want[0, 1].reshape(-1))


def test_parameter_sets_reach_the_branches_they_are_named_for():
    u = {s[0]: th.table_of(DT_UINT8, s[1], s[2]) for s in th.TABLE_SETS[DT_UINT8]}
    i = {s[0]: th.table_of(DT_INT8, s[1], s[2]) for s in th.TABLE_SETS[DT_INT8]}
    assert len(u) >= 8 and len(i) >= 8
    assert np.array_equal(u["equal"], np.arange(256, dtype=np.uint8)) and np.array_equal(u["equal_zp0"], np.arange(256, dtype=np.uint8))
    fine = u["finer_saturates_at_0_and_255"]
    assert (fine == 255).sum() > 1 and (fine == 0).sum() > 1 and fine[77] == 12
    assert (u["zp0_to_zp255"] == 255).all() and (u["zp255_to_zp0"] == 0).all()
    assert list(u["ties"][:8]) == [3, 3, 4, 4, 5, 5, 6, 6]                      # the double round(): ties away from zero
    # int8, indexed by the raw byte: byte 0x80 is -128.  Equal parameters: everything itself, but -128 -> -127
    ident = np.arange(256, dtype=np.uint8).view(np.int8).copy()
    ident[0x80] = -127
    assert np.array_equal(i["equal"], ident)
    for k in ("finer_saturates_at_pm127", "both_zp_nonzero_saturates"):
        assert i[k][0x80] == -127 and (i[k] == -127).sum() > 1 and (i[k] == 127).sum() > 1, k
    assert all((t != -128).all() for t in i.values())                            # -128 never comes out
    assert i["in_zp_nonzero"][9] == 0 and i["out_zp_nonzero"][0] == -11          # the zero points map onto each other
    assert list(i["ties"][:6]) == [3, 3, 4, 4, 5, 5] and list(i["ties"][0xfd:]) == [1, 2, 2]      # -3 -> (-6 * 0.5) + 4 = 1; -2 -> 1.5 -> 2


def test_transpose_table_refuses_what_the_reference_cannot_convert():
    for dt in (I8, U8):
        assert capi.transpose_table(dt, 0.05, 0, 0.0, 0) is None                 # x / 0: inf, or NaN for 0 / 0
        assert capi.transpose_table(dt, float("nan"), 0, 0.05, 0) is None and capi.transpose_table(dt, 0.05, 0, float("nan"), 0) is None
        assert capi.transpose_table(dt, float("inf"), 0, 0.05, 0) is None
        assert capi.transpose_table(dt, 1e30, 0, 1e-8, 0) is None                # inf, outside int
        assert capi.transpose_table(dt, 1.0, 0, 1e-8, 0) is None                 # 1.27e10: finite, outside int
        assert capi.transpose_table(dt, 1.0, 0, 1e-6, 0) is not None             # inside int, clamped
    assert capi.transpose_table(F32, 0.05, 0, 0.05, 0) is None and capi.transpose_table(FP16, 0.05, 0, 0.05, 0) is None


@pytest.mark.parametrize("dtype", [DT_UINT8, DT_INT8], ids=["u8", "i8"])
def test_identity_order_with_different_parameters_is_the_pure_map_not_a_copy(ref, dtype):
    g, x = T(dtype, (2, 3, 4, 5), (0, 1, 2, 3))
    q = lambda t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    assert q(0) != q(1)
    out = th.reference_outputs(ref, g, x, dtype)[0]
    assert out.shape == x.shape and not np.array_equal(out, x)
    assert np.array_equal(out, th.table_of(dtype, q(0), q(1))[x.view(np.uint8)])
    # .. and between EQUAL int8 parameters it still is not one: -128 comes out as -127
    if dtype == DT_INT8:
        g, x = T(dtype, (2, 3, 4, 5), (0, 1, 2, 3), (0.05, 0), (0.05, 0), force=-128)
        out = th.reference_outputs(ref, g, x, dtype)[0]
        assert (x == -128).any() and not (out == -128).any() and np.array_equal(out[x != -128], x[x != -128])


def _error(g):
    return th.library_outcome(tm2.write_tm2(g))[1]


def test_refused_forms_are_refused_by_name_when_a_file_carries_them():
    """through the tmfile reader and prerun's shape inference / validation, which run before the device is touched"""
    for dt in (DT_UINT8, DT_INT8):
        assert "1-D tensor" in _error(T(dt, (12,), (0,))[0])
        assert "more than 6 dimensions" in _error(T(dt, (1, 2, 1, 2, 1, 2, 3), (0, 1, 2, 3, 4, 5, 6))[0])
        assert "one entry per input dimension" in _error(T(dt, (2, 3, 4), (0, 1), out_dims=[2, 3])[0])
        assert "one entry per input dimension" in _error(T(dt, (2, 3), (0, 1, 1), out_dims=[2, 3, 3])[0])
        assert "repeats an axis" in _error(T(dt, (2, 3, 4), (0, 1, 1))[0])
        assert "outside the tensor's rank" in _error(T(dt, (2, 3, 4), (0, 1, 3), out_dims=[2, 3, 4])[0])
        assert "outside the tensor's rank" in _error(T(dt, (2, 3, 4), (0, -1, 2), out_dims=[2, 3, 4])[0])
        g, _ = T(dt, (2, 3, 4), (0, 2, 1))
        g.tensors[1].scales, g.tensors[1].zero_points = [lh.f32(0.03)] * 4, [0] * 4
        assert "per-tensor" in _error(g)
        g, _ = T(dt, (2, 3, 4), (0, 2, 1))
        g.tensors[0].scales, g.tensors[0].zero_points = [lh.f32(0.03)] * 3, [0] * 3
        assert "per-tensor" in _error(g)
        assert "cannot convert to int" in _error(T(dt, (2, 3, 4), (0, 2, 1), (1.0, 0), (1e-8, 0))[0])
        g = tm2.Graph(name="transpose_of_const")         # a Transpose that reads a constant tensor; the graph's input feeds nothing
        q = th.q_of(dt, (0.05, 0))
        g.add_input("data", [2, 3, 4], dt, *q)
        c = g.add_const("table", np.arange(24).reshape(2, 3, 4), dt, *q)
        y = g.add_tensor("out", [2, 4, 3], dt, tm2.TT_VAR, None, *q)
        g.output_nodes = [g.add_node("transpose", "Transpose", [c], [y], tr_shape=[0, 2, 1])]
        assert "must not be a constant" in _error(g)
        assert "transpose" not in _error(T(dt, (2, 3, 4), (0, 2, 1))[0]).lower()       # .. while a node that runs gets as far as the device
    assert "int8 and uint8 graphs only" in _error(T(DT_FP32, (2, 3, 4), (0, 2, 1))[0])


# what transpose_refusal answers (tests/csrc/transpose_rules_check.cc): (input line, expected output line).  The geometry is canonical:
# size-1 axes dropped, output axes that are neighbours in the input merged, (extent:input stride) in output order, the stride-1 axis
RULES = [
    ("u8 0 1 1 2 5 7 2 1 0", "OK out=7,5 geom=7:1,5:7 unit=0"),
    ("u8 0 1 1 3 2 5 7 3 0 2 1", "OK out=2,7,5 geom=2:35,7:1,5:7 unit=1"),
    ("u8 0 1 1 3 2 5 7 3 2 0 1", "OK out=7,2,5 geom=7:1,10:7 unit=0"),                              # (2, 5) are neighbours in the input: merged
    ("u8 0 1 1 3 2 5 7 3 1 0 2", "OK out=5,2,7 geom=5:7,2:35,7:1 unit=2"),
    ("i8 0 1 1 4 1 6 5 7 4 0 2 3 1", "OK out=1,5,7,6 geom=35:1,6:35 unit=0"),                       # NCHW -> NHWC at batch 1: a 2-D transpose
    ("u8 0 1 1 4 2 3 4 5 4 3 2 1 0", "OK out=5,4,3,2 geom=5:1,4:5,3:20,2:60 unit=0"),
    ("u8 0 1 1 4 2 3 4 5 4 0 1 3 2", "OK out=2,3,5,4 geom=6:20,5:1,4:5 unit=1"),
    ("u8 0 1 1 4 2 3 4 5 4 0 1 2 3", "OK out=2,3,4,5 geom=120:1 unit=0"),                           # the identity: one run
    ("u8 0 1 1 5 1 2 3 4 5 5 0 2 1 3 4", "OK out=1,3,2,4,5 geom=3:20,2:60,20:1 unit=2"),            # torch's channel shuffle
    ("i8 0 1 1 5 2 3 11 3 5 5 0 1 3 4 2", "OK out=2,3,3,5,11 geom=6:165,15:1,11:15 unit=1"),        # the Detect head: (anchors, 85, H * W) per image
    ("u8 0 1 1 6 1 2 3 2 3 5 6 0 1 4 2 5 3", "OK out=1,2,3,3,5,2 geom=2:90,3:5,3:30,5:1,2:15 unit=3"),
    ("u8 0 1 1 5 1 1 5 1 7 5 4 3 2 1 0", "OK out=7,1,5,1,1 geom=7:1,5:7 unit=0"),                   # size-1 axes drop out
    ("u8 0 1 1 3 2 3 1 3 1 0 2", "OK out=3,2,1 geom=3:1,2:3 unit=0"),                               # a run of one byte is no axis
    ("u8 0 1 1 2 1 1 2 1 0", "OK out=1,1 geom=1:1 unit=0"),                                         # one element
    ("u8 0 1 1 3 2 5 7 3 0 2 1 3 2 7 5", "OK out=2,7,5 geom=2:35,7:1,5:7 unit=1"),                  # the output's dims given, and right
    ("u8 0 1 1 3 2 5 7 3 0 2 1 3 2 5 7", "REFUSED Transpose: the output does not have the dims the reference infers"),
    ("u8 0 1 1 3 2 5 7 3 0 2 1 2 2 35", "REFUSED Transpose: the output does not have the dims the reference infers"),
    ("u8 0 1 1 3 2 5 7 -1", "REFUSED Transpose needs its parameter"),
    ("f32 0 1 1 3 2 5 7 3 0 2 1", "REFUSED Transpose runs on the device in int8 and uint8 graphs only"),
    ("u8 0 1 1 1 12 1 0", "REFUSED a Transpose of a 1-D tensor does not run on the device (the reference has no loop for rank 1)"),
    ("u8 0 1 1 7 1 2 1 2 1 2 3 7 0 1 2 3 4 5 6", "REFUSED a Transpose of a tensor of more than 6 dimensions does not run on the device (the reference has no loop above rank 6)"),
    ("u8 0 1 1 3 2 5 7 2 0 1", "REFUSED Transpose: tr_shape must have one entry per input dimension"),
    ("u8 0 1 1 2 5 7 3 0 1 1", "REFUSED Transpose: tr_shape must have one entry per input dimension"),
    ("u8 0 1 1 3 2 5 7 3 0 1 1", "REFUSED Transpose: tr_shape repeats an axis (it is not a permutation)"),
    ("u8 0 1 1 3 2 5 7 3 0 1 3", "REFUSED Transpose: a tr_shape entry is outside the tensor's rank"),
    ("u8 0 1 1 3 2 5 7 3 0 -1 2", "REFUSED Transpose: a tr_shape entry is outside the tensor's rank"),
    ("u8 1 1 1 3 2 5 7 3 0 2 1", "REFUSED Transpose: the input must not be a constant"),
    ("u8 0 3 1 3 2 5 7 3 0 2 1", "REFUSED Transpose needs per-tensor quant params on both sides"),
    ("i8 0 1 5 3 2 5 7 3 0 2 1", "REFUSED Transpose needs per-tensor quant params on both sides"),
    ("u8 0 1 1 3 2 0 7 3 0 2 1", "REFUSED Transpose: every input dimension must be at least 1"),
    ("bad 0 1 1 3 2 5 7 3 0 2 1", "REFUSED Transpose: the quantisation parameters give a value the reference cannot convert to int"),
]


def test_transpose_refusal_names_every_refusal_and_resolves_the_canonical_geometry(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "transpose_rules_check")
    subprocess.check_call([hipcc, "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tengine_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "transpose_rules_check.cc"), os.path.join(ROOT, "tengine_amd", "csrc", "transpose_tables.cc"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], input="\n".join(r[0] for r in RULES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(RULES), out.stdout
    for (case, want), got in zip(RULES, lines):
        assert got == want, (case, got, want)
    assert len({w for _, w in RULES if w.startswith("REFUSED")}) >= 11           # every refusal has its own reason


def test_support_queries():
    L = capi.lib()
    A = th.ask_transpose
    assert [L.tamd_op_supported(th.OP_TRANSPOSE, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 1, 1]
    for dt in (I8, U8):
        # what runs: every single-node case of the GPU tests, in both types
        for case, (dims, order, _, _) in th.U8_SINGLE.items():
            assert A(dt, list(dims), list(order)) == 1, case
        # .. and what does not, as the rule says
        assert A(dt, [12], [0]) == 0
        assert A(dt, [1, 2, 1, 2, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6]) == 0
        assert A(dt, [2, 3, 4], [0, 1], out_dims=[2, 3]) == 0 and A(dt, [2, 3], [0, 1, 1], out_dims=[2, 3, 3]) == 0
        assert A(dt, [2, 3, 4], [0, 1, 1]) == 0 and A(dt, [2, 3, 4], [0, 1, 3], out_dims=[2, 3, 4]) == 0 and A(dt, [2, 3, 4], [0, -1, 2], out_dims=[2, 3, 4]) == 0
        assert A(dt, [2, 3, 4], [0, 2, 1], const_input=True) == 0
        assert A(dt, [2, 3, 4], [0, 2, 1], in_quant=3) == 0 and A(dt, [2, 3, 4], [0, 2, 1], out_quant=4) == 0
        assert A(dt, [2, 3, 4], [0, 2, 1], out_dims=[2, 3, 4]) == 0 and A(dt, [2, 3, 4], [0, 2, 1], out_dims=[2, 12]) == 0
        assert A(dt, [2, 3, 4], [0, 2, 1], in_q=(1.0, 0), out_q=(1e-8, 0)) == 0 and A(dt, [2, 3, 4], [0, 2, 1], out_q=(0.0, 0)) == 0
        assert A(dt, [2, 3, 4], [0, 2, 1], with_param=False) == 0
    assert A(F32, [2, 3, 4], [0, 2, 1]) == 0
    # the operators that were there keep their answers and their codes; 21, 24 and 27 are reserved, never-supported values
    assert [L.tamd_op_supported(op, I8) for op in range(28)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0]
    assert [L.tamd_op_supported(op, U8) for op in range(28)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0]
    assert [L.tamd_op_supported(op, F32) for op in range(29)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert th.OP_TRANSPOSE == capi.OP_TRANSPOSE == 28
    assert [L.tamd_op_supported(29, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]


def test_writer_and_reader_round_trip_the_order_vector():
    for order in ([1, 0], [0, 2, 1], [0, 1, 3, 4, 2], [0, 1, 4, 2, 5, 3]):
        dims = [2, 3, 4, 5, 6, 7][:len(order)]
        g, _ = T(DT_UINT8, dims, order)
        b = tm2.write_tm2(g)
        node = [n for n in tm2.read_tm2(b).nodes if n.op == "Transpose"]
        assert len(node) == 1 and node[0].params == {"tr_shape": order}
        shape, err = th.library_outcome(b)                                       # tm2_reader.cc read the same vector: the shape it infers says so
        assert shape == tuple(dims[o] for o in order) and "transpose" not in err.lower(), (shape, err)
    # a node without the vector is refused by the reader
    g, _ = T(DT_UINT8, (2, 3, 4), None, out_dims=[2, 4, 3])
    b = tm2.write_tm2(g)
    assert [n for n in tm2.read_tm2(b).nodes if n.op == "Transpose"][0].params == {"tr_shape": None}
    L = capi.lib()
    assert not L.tamd_graph_load_tm2(b, len(b))
    assert "tr_shape" in L.tamd_last_error().decode()


@pytest.mark.parametrize("case", ["u8_5d_detect", "u8_6d", "i8_view", "i8_concat_view", "i8_detect", "u8_detect", "u8_shuffle", "u8_batch_axis"])
def test_written_tmfile_runs_in_the_reference(ref, case):
    """the reference loads a file tm2.py wrote and runs it (ranks 5 and 6 through Reshape -> Transpose -> Reshape included); the shape it
    infers is the one the library infers"""
    dtype, build = th.gpu_cases()[case]
    g, x = build()
    b = tm2.write_tm2(g)
    out = th.reference_outputs(ref, g, x, dtype)
    assert out[0].dtype == lh.NP[dtype]
    shape, err = th.library_outcome(b)
    assert shape == out[0].shape, (shape, out[0].shape, err)
    assert "not supported" not in err and "transpose" not in err.lower(), err


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("case", ["i8_detect", "u8_detect", "u8_shuffle"])
def test_plugin_keeps_the_block_in_one_hip_subgraph(ref, case):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    dtype, build = th.gpu_cases()[case]
    g, x = build()
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and {"Transpose", "Reshape", "Convolution"} <= set(real[0][1]), real


def test_plugin_leaves_the_refused_forms_and_fp32_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = th.Block(64, DT_FP32, (1, 8, 6, 6))
    c.conv(8, 3, 1); c.transpose((0, 1, 3, 2)); c.conv(8, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == ["Transpose"], real
    # int8: the convolution behind a Transpose reads a DENSE tensor, which the convolution stack does not: it stays on the CPU device
    c = th.Block(65, DT_INT8, (1, 8, 6, 6))
    c.conv(8, 3, 1); c.transpose((0, 1, 3, 2)); c.conv(8, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_INT8))
    assert [dev for dev, _ in real] == ["HIP", "CPU"] or [dev == "HIP" for dev, _ in real] == [True, False], real
    assert "Transpose" in real[0][1] and real[1][1] == ["Convolution"], real


def test_golden_is_the_real_reference(ref):
    """tests/golden/transpose_cases.npz (tests/transpose_helpers.py: write_golden) holds what the reference computes here, for every GPU
    case and table"""
    z = th.golden()
    cases = th.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    assert {k for k in z.files if k.startswith("table__")} == {th.table_key(dt, s[0]) for dt, sets in th.TABLE_SETS.items() for s in sets}
    assert os.path.getsize(th.GOLDEN) < 64 * 1024
    for case in sorted(stored):
        dtype, build = cases[case]
        g, x = build()
        want = th.reference_outputs(ref, g, x, dtype)
        assert th.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not th.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = th.gpu_cases()
    q = lambda g, t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    for k in ("u8_equal_params_tile", "u8_equal_params_rows", "i8_input_nhwc_minus128"):
        g, _ = cases[k][1]()
        assert q(g, 0) == q(g, 1), k
    for k in ("u8_4d_identity_order", "u8_2d", "u8_coarser", "i8_input_saturates"):
        g, _ = cases[k][1]()
        assert q(g, 0) != q(g, 1), k
    _, x = cases["i8_input_nhwc_minus128"][1]()
    assert (x == -128).sum() >= 7
    for k in ("i8_detect", "u8_detect"):
        g, _ = cases[k][1]()
        tr = [n for n in g.nodes if n.op == "Transpose"]
        assert len(tr) == 2 and all(n.params["tr_shape"] == [0, 1, 3, 4, 2] for n in tr)
        assert [g.tensors[n.outputs[0]].dims for n in tr] == [[2, 3, 4, 4, 7], [2, 3, 2, 2, 7]]
        assert sum(n.op == "Sigmoid" for n in g.nodes) == 2 and g.nodes[g.output_nodes[0]].op == "Concat"
    g, _ = cases["u8_batch_axis"][1]()
    assert all(t.dims[0] == 4 for t in g.tensors if t.ttype != tm2.TT_CONST)
    assert {len(th.TABLE_SETS[dt]) for dt in th.TABLE_SETS} == {8}
    sl = [(0.05, 77), (0.031, 12), (0.05, 0), (0.04, 255), (0.5, 3), (1.0, 4), (0.0173, 101), (0.0291, 37)]       # tests/slice_op_helpers.py: TABLE_SETS
    assert set(sl) <= {p for s in th.TABLE_SETS[DT_UINT8] for p in s[1:]}
