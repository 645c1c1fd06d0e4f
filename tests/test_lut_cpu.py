"""Quantised Sigmoid / Clip / HardSwish / Mish on the device, the parts that need no GPU: the tmfile writer and reader, the 256-entry
byte map of every (operator, type) pair against the real reference library on all 256 input bytes, what the support queries answer,
where the plugin's splitter puts the operators, and the table builders alone under the address / undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("op,dtype", lh.PAIRS, ids=["%s-%d" % p for p in lh.PAIRS])
def test_written_tmfile_loads_and_runs_in_the_reference(ref, op, dtype):
    """tm2.write_tm2 writes the operator and its parameter blob the way the reference's loader reads them; read_tm2 gives them back"""
    params = {"Clip": {"max": 2.5, "min": -0.75}, "HardSwish": {"alpha": 0.25, "beta": 0.5}}.get(op, {})
    g = lh.unary_graph(op, dtype, (1, 16, 4, 4), (0.05, 0 if dtype == DT_INT8 else 77), (0.031, 0 if dtype == DT_INT8 else 12), params)
    b = tm2.write_tm2(g)
    back = tm2.read_tm2(b)
    node = [n for n in back.nodes if n.op == op]
    assert len(node) == 1 and node[0].params == params
    out = ref.run_model(b, lh.all_bytes(dtype), lh.ref_mode(ref, dtype))
    assert len(out) == 1 and out[0].shape == (1, 16, 4, 4) and out[0].dtype == lh.NP[dtype]


@pytest.mark.parametrize("case", lh.PARAM_SETS, ids=[s[0] for s in lh.PARAM_SETS])
def test_table_is_the_reference_on_every_byte(ref, case):
    """the reference on a tensor that holds all 256 byte values, twice (it must be deterministic), against tamd_lut_table: byte equality"""
    _, op, dtype, in_q, out_q, params = case
    b = tm2.write_tm2(lh.unary_graph(op, dtype, (1, 16, 4, 4), in_q, out_q, params))
    x = lh.all_bytes(dtype)
    want = ref.run_model(b, x, lh.ref_mode(ref, dtype))[0]
    again = ref.run_model(b, x, lh.ref_mode(ref, dtype))[0]
    assert np.array_equal(want, again)
    got = lh.table_of(capi, op, dtype, in_q, out_q, params)
    assert got is not None and got.shape == (256,)
    assert np.array_equal(got, want.reshape(-1).view(np.uint8)), np.nonzero(got != want.reshape(-1).view(np.uint8))[0]


def test_parameter_sets_reach_the_branches_they_are_named_for(ref):
    """the sets are not vacuous: int8 Clip really wraps negative / passes 255, uint8 Clip really goes below 0, Sigmoid really leaves
    +-30, and 0 does not map to 0 for Sigmoid (the padding-lane trap of the device kernel)"""
    sets = {s[0]: s for s in lh.PARAM_SETS}

    def tab(name):
        _, op, dtype, in_q, out_q, params = sets[name]
        return lh.table_of(capi, op, dtype, in_q, out_q, params)

    assert (tab("clip6_i8_wraps_negative").view(np.int8) < 0).any() and tab("clip6_i8_wraps_negative").max() < 255
    assert (tab("clip6_i8_above_255") == 255).any()
    assert tab("clip_u8_below_0")[0] > 128                   # a negative quotient narrowed to uint8: no saturation at 0 in the reference
    assert tab("sigmoid_i8_a")[0] != 0 and tab("sigmoid_u8_zp0")[0] != 0
    assert abs(0.3 * 127) > 30
    assert np.array_equal(tab("hardswish_u8_zp77"), tab("hardswish_u8_alpha_beta_ignored"))


def test_support_queries():
    """tamd_op_supported / tamd_node_supported: Sigmoid and Clip in int8 and uint8, HardSwish and Mish in uint8 only, none in fp32;
    Mish on a 4-D tensor only"""
    L = capi.lib()
    F32, FP16, I8, U8 = 0, 1, 2, 3
    truth = {"Sigmoid": {I8: 1, U8: 1, F32: 0, FP16: 0}, "Clip": {I8: 1, U8: 1, F32: 0, FP16: 0},
             "HardSwish": {I8: 0, U8: 1, F32: 0, FP16: 0}, "Mish": {I8: 0, U8: 1, F32: 0, FP16: 0}}
    for op, row in truth.items():
        for dt, want in row.items():
            assert L.tamd_op_supported(lh.OPCODE[op], dt) == want, (op, dt)
            assert lh.ask_node(capi, op, dt, [1, 16, 4, 4]) == want, (op, dt)
            assert (lh.table_of(capi, op, dt, (0.05, 0), (0.02, 0), None) is not None) == bool(want), (op, dt)
    assert lh.ask_node(capi, "Mish", U8, [16, 4, 4]) == 0 and lh.ask_node(capi, "Mish", U8, [2, 40]) == 0
    for op in ("Sigmoid", "Clip", "HardSwish"):
        assert lh.ask_node(capi, op, U8, [16, 4, 4]) == 1 and lh.ask_node(capi, op, U8, [2, 40]) == 1, op
    assert lh.ask_node(capi, "Sigmoid", I8, [2, 40]) == 1
    assert lh.ask_node(capi, "Clip", I8, [1, 16, 4, 4], with_param=False) == 0
    # the operators that were there keep their answers and their codes
    assert [L.tamd_op_supported(op, I8) for op in range(16)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1]


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("build,dtype", [(lh.placement_a, DT_INT8), (lh.placement_b, DT_UINT8)], ids=["int8-clip-sigmoid", "uint8-mish-hardswish"])
def test_plugin_keeps_the_quantised_graph_in_one_hip_subgraph(ref, build, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = build(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and len(real[0][1]) == 4, real


@pytest.mark.parametrize("build,ops", [(lh.placement_a, {"Clip", "Sigmoid"}), (lh.placement_b, {"Mish", "HardSwish"})], ids=["clip-sigmoid", "mish-hardswish"])
def test_plugin_leaves_the_fp32_forms_to_the_cpu_device(ref, build, ops):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = build(DT_FP32)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    on_hip = {o for dev, os_ in real if dev == "HIP" for o in os_}
    on_cpu = {o.lower() for dev, os_ in real if dev != "HIP" for o in os_}       # (the reference spells it "Hardswish")
    assert on_hip == {"Convolution"} and on_cpu == {o.lower() for o in ops}, real


def test_int8_hardswish_and_mish_stay_on_the_cpu_device(ref):
    """the reference has no int8 kernel for them: nothing changes for such a graph (the splitter leaves the node where it was)"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = lh.Chain(31, DT_INT8, (1, 8, 6, 6))
    c.conv(16, 3, 1); c.act("HardSwish", (0.03, 0)); c.conv(12, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_INT8))
    assert [o.lower() for dev, os_ in real if dev != "HIP" for o in os_] == ["hardswish"], real


def test_table_builders_alone_under_the_sanitizers(tmp_path):
    """tests/csrc/lut_tables_check.cc + csrc/lut_tables.cc and nothing else, built with -fsanitize=address,undefined: every parameter
    set's table is built, the program exits 0, and its tables are the library's (another compiler, the same bytes)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lut_tables_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "lut_tables_check.cc"), os.path.join(ROOT, "tengine_amd", "csrc", "lut_tables.cc"),
                           "-lm", "-o", exe])
    hexf = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]
    args = []
    for _, op, dtype, in_q, out_q, params in lh.PARAM_SETS:
        p = lh.DEFAULT_PARAMS[op] if params is None else params
        pair = (p["max"], p["min"]) if op == "Clip" else (p["alpha"], p["beta"]) if op == "HardSwish" else (0.0, 0.0)
        args += [str(lh.OPCODE[op]), str(dtype), hexf(in_q[0]), str(in_q[1]), hexf(out_q[0]), str(out_q[1]), hexf(pair[0]), hexf(pair[1])]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split()
    assert len(lines) == len(lh.PARAM_SETS)
    for line, (_, op, dtype, in_q, out_q, params) in zip(lines, lh.PARAM_SETS):
        assert np.array_equal(np.frombuffer(bytes.fromhex(line), np.uint8), lh.table_of(capi, op, dtype, in_q, out_q, params)), op
