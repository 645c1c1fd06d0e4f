"""Quantised PReLU on the device, the parts that need no GPU: the half-widening routine against the built reference's own symbol on
all 65 536 patterns, the per-channel byte table against the real reference library on all 256 input bytes, what the support queries
answer and what prerun refuses (each form by its own name), where the plugin's splitter puts the node, the committed golden against
the reference, and the host code alone under the address / undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lut_helpers as lh
import prelu_helpers as ph
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP16, DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3


def _bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def test_widening_is_the_built_references_on_every_half(ref):
    """all 65 536 half patterns through tamd_prelu_slope against fp16_to_fp32 of the BUILT reference library (a 2-byte struct by value
    in, a float out), by bit pattern.  The normal halves whose fraction is zero fall through every branch of that routine and come out
    as whatever its object code leaves in the register: +0.0f as built here.  A build that decides otherwise fails HERE."""
    class Half(C.Structure):
        _fields_ = [("bits", C.c_uint16)]
    widen = ref.lib().fp16_to_fp32
    widen.argtypes, widen.restype = [Half], C.c_float
    mine = capi.lib().tamd_prelu_slope
    want = np.array([widen(Half(h)) for h in range(65536)], np.float32).view(np.uint32)
    got = np.array([mine(h) for h in range(65536)], np.float32).view(np.uint32)
    assert np.array_equal(want, got), [hex(h) for h in np.nonzero(want != got)[0][:8]]
    assert _bits(capi.prelu_slope(0x3400)) == 0                       # 0.25 widens to +0.0f: a PReLU with the customary slope is a ReLU
    assert _bits(capi.prelu_slope(0xb400)) == 0 and _bits(capi.prelu_slope(0x3c00)) == 0 and _bits(capi.prelu_slope(0x4400)) == 0
    assert _bits(capi.prelu_slope(0x0003)) == 0x34000200 and _bits(capi.prelu_slope(0x8000)) == 0x80000000
    assert _bits(capi.prelu_slope(0x7c00)) == 0x7f800000 and np.isnan(capi.prelu_slope(0x7e00))      # (fraction 1, a signalling NaN: ctypes quiets it on both sides)
    ieee = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
    nan = np.isnan(ieee.view(np.float32))
    assert int((got != ieee)[~nan].sum()) + int(nan.sum()) == 4132    # 60 powers of two, 2026 sub-normals, 2046 NaNs (fraction 1)
    assert np.float32(capi.prelu_slope(ph.half(0.1))) == np.float16(0.1).astype(np.float32)


@pytest.mark.parametrize("case", ph.ALL_BYTES_SETS, ids=[s[0] for s in ph.ALL_BYTES_SETS])
def test_table_is_the_reference_on_every_byte(ref, case):
    """the reference on (1, C, 16, 16) where every channel holds all 256 byte values, twice (it must be deterministic), against
    tamd_prelu_table of every channel: byte equality"""
    _, dtype, c, in_q, out_q, shared = case
    g, x, bits = ph.all_bytes_case(case)
    assert len(bits) == c
    b = tm2.write_tm2(g)
    back = tm2.read_tm2(b)
    assert [n.op for n in back.nodes if n.op not in ("InputOp", "Const")] == ["PReLU"]
    want = ref.run_model(b, x, lh.ref_mode(ref, dtype))[0]
    again = ref.run_model(b, x, lh.ref_mode(ref, dtype))[0]
    assert want.shape == (1, c, 16, 16) and want.dtype == lh.NP[dtype] and np.array_equal(want, again)
    got = ph.expected_all_bytes(case)
    assert np.array_equal(got, want), [(ch, int((got[0, ch] != want[0, ch]).sum())) for ch in range(c) if (got[0, ch] != want[0, ch]).any()]


def test_parameter_sets_reach_the_branches_they_are_named_for():
    name = {n: b for n, b in ph.SLOPES}
    i8 = lambda b, out=0.031: capi.prelu_table(I8, b, lh.f32(0.05), 0, lh.f32(out), 0).view(np.int8)
    relu = i8(name["zero"])
    assert (relu[128:] == 0).all() and relu[1] > 0
    for acts_as_0 in ("quarter_acts_as_0", "four_acts_as_0", "minus_zero", "subnormal"):
        assert np.array_equal(i8(name[acts_as_0]), relu), acts_as_0
    assert (i8(name["tenth"])[128:] < 0).any() and (i8(name["negative"])[128:254] > 0).all()
    sat = i8(name["saturates"])
    assert sat.min() == -127 and sat.max() == 127 and sat[128] == -127 and (sat != -128).all()       # -128 in never comes out as -128
    assert (i8(name["tenth"], 0.0031)[129:] == -127).sum() > 1 and (i8(name["tenth"], 0.0031) != -128).all()
    for zp in (0, 128, 255):
        u8 = capi.prelu_table(U8, name["saturates"], lh.f32(0.05), zp, lh.f32(0.02), 100)
        assert u8[zp] == 100 and (zp == 0 or u8[0] == 0) and (zp == 255 or u8[255] == 255), zp
    # every slope of the set is in every all-bytes case with 16 and 20 channels, and in the 5-channel ones the first five
    assert set(ph.slopes_for(16)) == set(ph.SLOPE_BITS) and len(ph.SLOPE_BITS) == 8
    assert {s[2] for s in ph.ALL_BYTES_SETS} == {5, 16, 20}
    u8sets = [s for s in ph.ALL_BYTES_SETS if s[1] == DT_UINT8]
    assert {s[3][1] for s in u8sets} >= {0, 128, 255} and all(s[3][1] != s[4][1] for s in u8sets) and any(s[5] is not None for s in u8sets)


def test_support_queries():
    L = capi.lib()
    assert [L.tamd_op_supported(ph.OP_PRELU, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 1, 1]
    for reserved in (21, 24):
        assert [L.tamd_op_supported(reserved, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]
    assert L.tamd_op_supported(26, I8) == 0
    for dt in (I8, U8):                  # PReLU is no function of one byte and two quantisation pairs: it has its own entry points
        assert capi.lut_table(ph.OP_PRELU, dt, lh.f32(0.05), 0, lh.f32(0.02), 0) is None
    assert capi.prelu_table(F32, 0x2e66, 0.05, 0, 0.02, 0) is None and capi.prelu_table(FP16, 0x2e66, 0.05, 0, 0.02, 0) is None
    assert capi.prelu_table(I8, 0x7c00, 0.05, 0, 0.02, 0) is None and capi.prelu_table(U8, 0x7e00, 0.05, 0, 0.02, 0) is None
    # what runs
    five = ph.slopes_for(5)
    assert ph.ask_node(I8, [1, 5, 4, 4], five) == 1 and ph.ask_node(U8, [2, 5, 7, 7], five) == 1
    assert ph.ask_node(U8, [2, 5, 7, 7], [0x2e66]) == 1                                  # uint8: one slope for all
    assert ph.ask_node(I8, [1, 5, 4, 4], five, with_payload=False) == 1                   # (descriptors alone: the values are not known)
    # .. and what does not, each for its own reason (the names: test_refused_forms_are_refused_by_name)
    assert ph.ask_node(I8, [5, 4, 4], five) == 0 and ph.ask_node(U8, [5, 4, 4], five) == 0          # 3-D
    assert ph.ask_node(I8, [4, 5], five) == 0 and ph.ask_node(U8, [4, 5], five) == 0                # 2-D
    assert ph.ask_node(I8, [1, 5, 4, 4], [0x2e66]) == 0                                   # int8: a shared slope
    assert ph.ask_node(I8, [1, 5, 4, 4], ph.slopes_for(4)) == 0 and ph.ask_node(I8, [1, 5, 4, 4], ph.slopes_for(6)) == 0
    assert ph.ask_node(U8, [1, 5, 4, 4], ph.slopes_for(2)) == 0 and ph.ask_node(U8, [1, 5, 4, 4], ph.slopes_for(6)) == 0
    assert ph.ask_node(I8, [1, 5, 4, 4], five, slope_const_=False) == 0
    assert ph.ask_node(I8, [1, 5, 4, 4], five, slope_dtype=DT_FP32) == 0 and ph.ask_node(U8, [1, 5, 4, 4], five, slope_dtype=DT_UINT8) == 0
    assert ph.ask_node(I8, [1, 5, 4, 4], [0x7c00] + five[1:]) == 0 and ph.ask_node(U8, [1, 5, 4, 4], five[:4] + [0xfe01]) == 0       # inf; NaN
    assert ph.ask_node(I8, [1, 5, 4, 4], five, in_quant=5) == 0 and ph.ask_node(U8, [1, 5, 4, 4], five, out_quant=5) == 0
    assert ph.ask_node(I8, [1, 5, 4, 4], five, const_input=True) == 0
    assert ph.ask_node(F32, [1, 5, 4, 4], five) == 0 and ph.ask_node(F32, [1, 5, 4, 4], five, slope_dtype=DT_FP32) == 0
    assert ph.ask_node(I8, [1, 5, 4, 4], five, inputs=1) == 0
    # the operators that were there keep their answers and their codes
    assert [L.tamd_op_supported(op, I8) for op in range(24)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1]
    assert [L.tamd_op_supported(op, U8) for op in range(24)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1]
    assert [L.tamd_op_supported(op, F32) for op in range(24)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]


def _multi_quant(g, name, n):
    t = [t for t in g.tensors if t.name == name][0]
    t.scales, t.zero_points = [t.scales[0]] * n, [t.zero_points[0]] * n


def test_refused_forms_are_refused_by_name():
    """through the tmfile reader and prerun's validation (which run before the device is touched): every form the reference does not
    define, by its own reason"""
    five = ph.slopes_for(5)
    q8, qo8, qu, quo = (0.05, 0), (0.031, 0), (0.05, 77), (0.031, 12)
    err = lambda g: ph.library_error(tm2.write_tm2(g))
    assert "4-D tensor only" in err(ph.unary_graph(DT_INT8, (5, 4, 4), q8, qo8, five))
    assert "4-D tensor only" in err(ph.unary_graph(DT_UINT8, (5, 4, 4), qu, quo, five))
    assert "4-D tensor only" in err(ph.unary_graph(DT_UINT8, (4, 5), qu, quo, five))
    assert "int8 PReLU needs one slope per channel" in err(ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, [0x2e66]))
    assert "int8 PReLU needs one slope per channel" in err(ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, ph.slopes_for(6)))
    assert "uint8 PReLU needs one slope per channel, or one for all" in err(ph.unary_graph(DT_UINT8, (1, 5, 4, 4), qu, quo, ph.slopes_for(3)))
    assert "must be fp16" in err(ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, five, slope_dtype=DT_FP32))
    assert "widens to inf or NaN" in err(ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, five[:4] + [0xfc00]))
    assert "widens to inf or NaN" in err(ph.unary_graph(DT_UINT8, (1, 5, 4, 4), qu, quo, [0x7e00]))
    assert "int8 and uint8 graphs only" in err(ph.unary_graph(DT_FP32, (1, 5, 4, 4), None, None, five, slope_dtype=DT_FP32))
    g = ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, five)
    _multi_quant(g, "data", 5)
    assert "per-tensor quant params on its input" in err(g)
    g = ph.unary_graph(DT_UINT8, (1, 5, 4, 4), qu, quo, five)
    _multi_quant(g, "out", 5)
    assert "per-tensor quant params on its output" in err(g)
    # a slope that is not a constant: the second input is another variable tensor
    g = ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, five)
    other = g.add_input("slope_in", [5], DT_FP16)
    [n for n in g.nodes if n.op == "PReLU"][0].inputs[1] = other
    assert "slope must be a constant" in err(g)
    # a constant data tensor
    g = ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, five)
    const = g.add_const("frozen", np.zeros((1, 5, 4, 4), np.int8), DT_INT8, [lh.f32(0.05)], [0])
    [n for n in g.nodes if n.op == "PReLU"][0].inputs[0] = const
    assert "must not be a constant" in err(g)
    # .. and what runs is not refused: validation passes, and prerun gets as far as the device (or through, where there is one)
    ok = err(ph.unary_graph(DT_INT8, (1, 5, 4, 4), q8, qo8, five))
    assert "PReLU" not in ok and "prelu" not in ok, ok


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_keeps_the_quantised_bottleneck_in_one_hip_subgraph(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ph.bottleneck_graph(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP", real
    assert sorted(real[0][1]) == ["Convolution"] * 3 + ["Eltwise"] + ["PReLU"] * 2, real


def test_plugin_leaves_the_fp32_prelu_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = ph.bottleneck_graph(DT_FP32)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    on_hip = {o for dev, os_ in real if dev == "HIP" for o in os_}
    on_cpu = [o for dev, os_ in real if dev != "HIP" for o in os_]
    assert "PReLU" not in on_hip and on_cpu.count("PReLU") == 2 and "Convolution" in on_hip, real


def test_plugin_leaves_a_nan_slope_to_the_cpu_device(ref):
    """the splitter asks with the slope's values, so that it and prerun cannot disagree"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = ph.Face(53, DT_INT8, (1, 8, 6, 6))
    c.conv(16, 1); c.prelu(bits=[0x7e00] + ph.slopes_for(15)); c.conv(8, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_INT8))
    assert [o for dev, os_ in real if dev != "HIP" for o in os_] == ["PReLU"], real


def test_quarter_slope_is_a_relu_in_the_reference(ref):
    gp, gr, x = ph.quarter_and_relu_graphs(DT_INT8)
    a = ref.run_model(tm2.write_tm2(gp), x, ref.MODE_INT8)[0]
    b = ref.run_model(tm2.write_tm2(gr), x, ref.MODE_INT8)[0]
    assert (x < 0).any() and np.array_equal(a, b) and (a[x < 0] == 0).all()


def test_golden_is_the_real_reference(ref):
    """tests/golden/prelu_cases.npz (tools/make_golden_prelu.py) holds the input of every GPU case and what the reference computes
    from it"""
    z = ph.golden()
    cases = ph.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    assert os.path.getsize(ph.GOLDEN) < 64 * 1024
    for case in sorted(stored):
        dtype, build = cases[case]
        g, x = build()
        assert z[case + "__in"].dtype == x.dtype and np.array_equal(z[case + "__in"], x), case
        want = ph.reference_outputs(ref, g, x, dtype)
        assert ph.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not ph.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = ph.gpu_cases()
    _, x = cases["i8_batch2_minus128"][1]()
    assert (x == -128).sum() >= 2 and x.shape[0] == 2
    g, x = cases["u8_planes_49_bytes_batch2"][1]()
    assert x.shape[2] * x.shape[3] == 49 and x.shape[0] * x.shape[1] > 2
    g, _ = cases["u8_planes_shared_slope"][1]()
    assert [t for t in g.tensors if t.name == "slope"][0].dims == [1]
    for k in ("i8_bottleneck", "u8_bottleneck"):
        g, x = cases[k][1]()
        assert [n.op for n in g.nodes if n.op not in ("InputOp", "Const")] == ["Convolution", "PReLU", "Convolution", "PReLU", "Convolution", "Eltwise"]
        assert tuple(x.shape) == (1, 8, 8, 8)
        for n in g.nodes:
            if n.op == "PReLU":
                s = g.tensors[n.inputs[1]]
                assert s.dtype == DT_FP16 and s.dims == [16] and int(np.asarray(s.data).view(np.uint16)[0]) == 0x3400


def test_host_code_alone_under_the_sanitizers(tmp_path):
    """tests/csrc/prelu_tables_check.cc + csrc/prelu_tables.cc and nothing else, built with -fsanitize=address,undefined and run as a
    plain child process: every parameter set's tables and the degenerate ones are built, all 65 536 halves are widened, the program
    exits 0, and its tables are the library's (another compiler, the same bytes)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "prelu_tables_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "prelu_tables_check.cc"), os.path.join(ROOT, "tengine_amd", "csrc", "prelu_tables.cc"),
                           "-lm", "-o", exe])
    hexf = lambda v: "%08x" % _bits(lh.f32(v))
    args, want = [], []
    for _, dtype, c, in_q, out_q, shared in ph.ALL_BYTES_SETS:
        for b in (ph.SLOPE_BITS if shared is None else [shared]):
            args += [str(dtype), "%04x" % b, hexf(in_q[0]), str(in_q[1]), hexf(out_q[0]), str(out_q[1])]
            want.append(capi.prelu_table(dtype, b, lh.f32(in_q[0]), in_q[1], lh.f32(out_q[0]), out_q[1]).tobytes().hex())
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert lines[:-1] == want and lines[-1] == "differ 4132 nonfinite 2048"
