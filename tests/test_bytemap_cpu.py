"""Eltwise with a constant scalar and the unary Eltwise types on the device by table, the parts that need no GPU: tamd_eltwise_table
against the real reference library on all 256 input bytes for every (type, data type) pair that runs, tamd_eltwise_pair on all 65 536
byte pairs, the committed golden against the reference, every refusal by its own name, the tmfile round trip of a one-input Eltwise,
where the plugin's splitter puts the nodes, and the table builders alone under the address / undefined-behaviour sanitizers.
Equality is of bytes everywhere: there is no tolerance in this file."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bytemap_helpers as bh
import lut_helpers as lh
import se_helpers as sh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", bh.PARAM_SETS, ids=[s[0] for s in bh.PARAM_SETS])
def test_table_is_the_reference_on_every_byte(ref, case):
    """the reference's CPU device on a (1, 4, 8, 8) tensor that holds every byte once, twice (it must be deterministic), against
    tamd_eltwise_table"""
    _, typ, dtype, in_q, out_q, const, params = case
    b = tm2.write_tm2(bh.node_graph(dtype, typ, (1, 4, 8, 8), in_q, out_q, const, params))
    x = bh.all_bytes(dtype)
    want = ref.run_model(b, x, lh.ref_mode(ref, dtype))[0]
    again = ref.run_model(b, x, lh.ref_mode(ref, dtype))[0]
    assert want.shape == (1, 4, 8, 8) and want.dtype == lh.NP[dtype] and np.array_equal(want, again)
    rc, got = bh.table_of(typ, dtype, in_q, out_q, const, params)
    assert rc == 0 and got.shape == (256,)
    w = want.reshape(-1).view(np.uint8)
    assert np.array_equal(got, w), np.nonzero(got != w)[0]


def test_parameter_sets_cover_what_they_must():
    """at least eight sets per running pair; every scalar pair has a set that saturates at BOTH ends (several bytes each) and every
    unary pair one that saturates at the top -- LOG, FLOOR and POWER, which can be negative, at both ends too --; uint8 graphs take
    fp32 and uint8 constants, int8 graphs int8 ones, -128 among them; the input holds int8 -128; SUB is not SUM and byte 0 does not map to byte 0 everywhere (the padding-lane trap of lut_u8)"""
    per = {}
    for s in bh.PARAM_SETS:
        per.setdefault((s[1], s[2]), []).append(s)
    assert sorted(per) == bh.RUNNING_PAIRS and len(per) == 7 * 2 + 7 + 4
    assert (bh.all_bytes(DT_INT8) == -128).sum() == 1
    for (typ, dtype), sets in per.items():
        assert len(sets) >= 8, (typ, dtype)
        lo, hi = (-127, 127) if dtype == DT_INT8 else (0, 255)
        both = top = False
        for _, _, _, iq, oq, const, params in sets:
            rc, t = bh.table_of(typ, dtype, iq, oq, const, params)
            assert rc == 0
            v = t.view(np.int8) if dtype == DT_INT8 else t
            assert v.min() >= lo
            both = both or ((v == lo).sum() > 1 and (v == hi).sum() > 1)
            top = top or (v == hi).sum() > 1
        # (LOG, FLOOR and POWER reach below zero too; RSQRT, EXP, SQRT and SQUARE are never negative, so with a zero point >= 0 they
        # have no low end to pass)
        assert both if typ in bh.SCALAR_TYPES.values() or typ in (11, 14, 17) else top, (typ, dtype)
        if typ in bh.SCALAR_TYPES.values():
            kinds = {s[5][0] for s in sets}
            assert kinds == ({"u8", "f32"} if dtype == DT_UINT8 else {"i8"}), (typ, dtype, kinds)
    assert any(s[5] is not None and s[5][0] == "i8" and s[5][1] == -128 for s in bh.PARAM_SETS)
    sets = {s[0]: s for s in bh.PARAM_SETS}
    tab = lambda name: bh.table_of(*sets[name][1:])[1]
    assert not np.array_equal(tab("sum_u8_1"), tab("sub_u8_1")) and tab("sum_i8_0")[0] != 0


PAIR_TYPES = {"prod": 0, "sum": 2, "sub": 4, "max": 6}


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("typ", sorted(PAIR_TYPES))
def test_pair_is_the_reference_on_every_byte_pair(ref, dtype, typ):
    """the same-shape form on two (1, 256, 16, 16) tensors -- every channel of a holds all 256 values, channel c of b holds byte c -- against
    tamd_eltwise_pair on all 65 536 pairs"""
    qx, qg, qo = sh.QUANT[dtype]
    out_q = qo.get(typ, (0.02, 0 if dtype == DT_INT8 else 128))      # (MAX: [-2.56, 6.35] | [-2.8, 7.75] in steps of 0.02 passes both ends)
    g = sh.gate_graph(dtype, PAIR_TYPES[typ] if typ == "max" else typ, (1, 256, 16, 16), (1, 256, 16, 16), out_q=out_q)
    a = sh.all_pairs_inputs(dtype)[0]
    b = np.repeat(np.arange(256, dtype=np.uint8), 256).view(lh.NP[dtype]).reshape(1, 256, 16, 16)
    want = sh.reference_outputs(ref, g, [a, b], dtype)[0].reshape(-1).view(np.uint8)
    f = lambda q: (lh.f32(q[0]), int(q[1]))
    L = capi.lib()
    code, (sa, za), (sb, zb), (so, zo) = PAIR_TYPES[typ], f(qx), f(qg), f(out_q)
    got = np.array([L.tamd_eltwise_pair(code, dtype, int(x), sa, za, int(y), sb, zb, so, zo) for x, y in zip(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))])
    assert got.min() >= 0 and np.array_equal(got.astype(np.uint8), want), int((got != want).sum())
    v = want.view(np.int8) if dtype == DT_INT8 else want
    assert (v.min(), v.max()) == ((-127, 127) if dtype == DT_INT8 else (0, 255))


def test_golden_is_the_real_reference(ref):
    """tests/golden/bytemap_cases.npz (tools/make_golden_bytemap.py) holds the inputs of every GPU case and what the reference computes
    from them, and nothing else"""
    z = bh.golden()
    cases = bh.gpu_cases()
    assert {k[:-3] for k in z.files if k.endswith("__n")} == set(cases)
    assert os.path.getsize(bh.GOLDEN) < 128 * 1024
    for case in sorted(cases):
        dtype, build = cases[case]
        g, xs = build()
        assert int(z[case + "__nin"]) == len(xs)
        for i, x in enumerate(xs):
            assert z["%s__in%d" % (case, i)].dtype == x.dtype and np.array_equal(z["%s__in%d" % (case, i)], x), case
        want = bh.reference_outputs(ref, g, xs, dtype)
        assert bh.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1
        assert not bh.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = bh.gpu_cases()
    assert len([c for c in cases if c.startswith("all_")]) == len(bh.RUNNING_PAIRS) == len([c for c in cases if c.startswith("ragged_")])
    g, xs = cases["ragged_i8_sum"][1]()
    assert xs[0].shape == (2, 5, 3, 3) and xs[0].size % 16 != 0
    for dt in ("i8", "u8"):
        g, _ = cases[dt + "_normalise"][1]()
        assert [(n.op, n.params.get("type")) for n in g.nodes if n.op not in ("InputOp", "Const")][:2] == [("Eltwise", 5), ("Eltwise", 1)]
        g, _ = cases[dt + "_hardswish"][1]()
        ops = [(n.op, n.params.get("type")) for n in g.nodes if n.op not in ("InputOp", "Const")]
        assert ops == [("Convolution", None), ("Eltwise", 2), ("Clip", None), ("Eltwise", 0), ("Eltwise", 1), ("Convolution", None)]
    g, _ = cases["u8_hardswish_div"][1]()
    assert [n.params["type"] for n in g.nodes if n.op == "Eltwise"] == [2, 0, 10]
    g, _ = cases["u8_normalise"][1]()
    consts = [g.tensors[n.inputs[1]] for n in g.nodes if n.op == "Eltwise"]
    assert [t.dtype for t in consts] == [DT_FP32, DT_FP32] and [float(t.data.reshape(-1)[0]) for t in consts] == [127.5, 0.0078125]
    g, _ = cases["i8_padding"][1]()
    e = [n for n in g.nodes if n.op == "Eltwise"][0]
    assert g.tensors[e.inputs[0]].dims[1] == 5
    t = g.tensors
    rc, tab = capi.eltwise_table(2, DT_INT8, capi.eltwise_scalar(DT_INT8, t[e.inputs[1]].data, t[e.inputs[1]].scales[0], 0), t[e.inputs[0]].scales[0], 0, t[e.outputs[0]].scales[0], 0)
    assert rc == 0 and tab[0] != 0                           # a padding lane mapped through the table would not stay zero


def test_support_query_accepts_the_forms_that_run():
    """tamd_node_supported answers 1 (0 before the feature existed) with and without the values handed over; prerun's validation lets the
    node through and gets as far as the device"""
    for _, typ, dtype, in_q, out_q, const, params in bh.PARAM_SETS[::3]:
        assert bh.ask_node(dtype, typ, [2, 5, 3, 3], const, params=params) == 1, (typ, dtype)
        assert bh.ask_node(dtype, typ, [2, 5, 3, 3], const, in_q, out_q, params) == 1, (typ, dtype)
        err = bh.library_error(tm2.write_tm2(bh.node_graph(dtype, typ, (2, 5, 3, 3), in_q, out_q, const, params)))
        assert "ltwise" not in err, err
    # a one-element constant of any rank, and x of one element or one plane
    assert bh.ask_node(DT_UINT8, 1, [2, 5, 3, 3], ("f32", 0.5, [1, 1, 1, 1])) == 1
    assert bh.ask_node(DT_INT8, 4, [1, 1, 1, 1], ("i8", 3, 0.5)) == 1 and bh.ask_node(DT_UINT8, 4, [1, 1, 3, 3], ("u8", 3, 0.5, 1)) == 1


# (what it is, node_graph arguments, part of the reason prerun's validation gives); dtype None: int8 and uint8
U8_C, I8_C = ("u8", 140, 0.05, 128), ("i8", 12, 0.05)
REFUSED = [
    ("sum_scalar", None, dict(typ=3), "SUM_SCALAR"),
    ("sum_scalar_says_scalar_and_unary", None, dict(typ=3), "scalar and unary"),
    ("max_with_a_scalar", None, dict(typ=6), "MAX with a one-element operand"),
    ("pow", None, dict(typ=16), "POW does not run on the device"),
    ("pow_unary", None, dict(typ=16, const=None), "POW does not run on the device"),
    ("last", None, dict(typ=9), "LAST is no operator"),
    ("scalar_not_constant", None, dict(typ=2, const_is_input=True), "one-element operand"),
    ("scalar_type_not_constant", None, dict(typ=5, const_is_input=True), "one-element operand that is not a constant"),
    ("constant_first", None, dict(typ=4, const_first=True), "constant is listed first"),
    ("x_2d", None, dict(typ=1, dims=(4, 9)), "take a 4-D activation"),
    ("x_3d", None, dict(typ=2, dims=(4, 3, 3)), "take a 4-D activation"),
    ("x_5d", None, dict(typ=2, dims=(1, 2, 2, 3, 3)), "take a 4-D activation"),
    ("unary_3d", None, dict(typ=15, const=None, dims=(4, 3, 3)), "take a 4-D activation"),
    ("unary_type_with_two_inputs", None, dict(typ=13), "a unary type takes one input"),
    ("scalar_type_with_one_input", None, dict(typ=5, const=None), "on two tensors"),
    ("binary_type_with_one_input", None, dict(typ=2, const=None), "on two tensors"),
    ("fp32_constant_in_int8", DT_INT8, dict(typ=1, const=("f32", 0.5)), "an fp32 constant does not run on the device"),
    ("uint8_constant_in_int8", DT_INT8, dict(typ=1, const=U8_C), "int8 in an int8 graph"),
    ("int8_constant_in_uint8", DT_UINT8, dict(typ=1, const=I8_C), "uint8 or fp32 in a uint8 graph"),
    ("rsqrt_of_zero", DT_UINT8, dict(typ=7, const=None, in_q=(0.05, 0)), "a value the reference does not define"),
    ("rsqrt_of_zero_inside", DT_UINT8, dict(typ=7, const=None, in_q=(0.05, 128)), "a value the reference does not define"),
    ("log_of_zero", DT_UINT8, dict(typ=11, const=None, in_q=(0.05, 0)), "a value the reference does not define"),
    ("sqrt_of_negative", DT_UINT8, dict(typ=13, const=None, in_q=(0.05, 1)), "a value the reference does not define"),
    ("int8_rsqrt", DT_INT8, dict(typ=7, const=None), "a value the reference does not define"),
    ("int8_log", DT_INT8, dict(typ=11, const=None), "a value the reference does not define"),
    ("int8_sqrt", DT_INT8, dict(typ=13, const=None), "a value the reference does not define"),
    ("division_by_zero", DT_UINT8, dict(typ=10, const=("f32", 0.0)), "a value the reference does not define"),
    ("division_by_a_zero_byte", DT_INT8, dict(typ=10, const=("i8", 0, 0.05)), "a value the reference does not define"),
    ("exp_overflows", DT_UINT8, dict(typ=12, const=None, in_q=(1.0, 0)), "a value the reference does not define"),
    ("outside_int", DT_UINT8, dict(typ=1, const=("f32", 1.0e9), in_q=(1.0, 0), out_q=(0.001, 0)), "a value the reference does not define"),
    ("power_fractional_of_negative", DT_UINT8, dict(typ=17, const=None, in_q=(0.05, 128), params={"shift": 0.0, "scale": 1.0, "power": 0.5}), "a value the reference does not define"),
]


@pytest.mark.parametrize("row", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_forms_are_refused_by_name(row):
    """tamd_node_supported answers 0 (with the values handed over, as the plugin does), and prerun's validation, which runs before the
    device is touched, names the reason"""
    _, only, kw, reason = row
    for dt in ((DT_INT8, DT_UINT8) if only is None else (only,)):
        k = dict(kw)
        typ, dims = k.pop("typ"), k.pop("dims", (2, 5, 3, 3))
        const = k.pop("const", I8_C if dt == DT_INT8 else U8_C)
        in_q = k.pop("in_q", (0.05, 0 if dt == DT_INT8 else 128))
        out_q = k.pop("out_q", (0.05, 0 if dt == DT_INT8 else 128))
        params = k.pop("params", None)
        assert bh.ask_node(dt, typ, list(dims), const, in_q, out_q, params, const_first=k.get("const_first", False), const_var=k.get("const_is_input", False)) == 0
        err = bh.library_error(tm2.write_tm2(bh.node_graph(dt, typ, dims, in_q, out_q, const, params, **k)))
        assert reason in err, err


def test_refused_quantisation_and_fp32_graphs():
    for dt in (DT_INT8, DT_UINT8):
        c = I8_C if dt == DT_INT8 else U8_C
        assert bh.ask_node(dt, 1, [2, 5, 3, 3], c, x_quant=5) == 0 and bh.ask_node(dt, 1, [2, 5, 3, 3], c, out_quant=5) == 0
        assert bh.ask_node(dt, 15, [2, 5, 3, 3], x_quant=5) == 0 and bh.ask_node(dt, 15, [2, 5, 3, 3], out_quant=5) == 0
        assert bh.ask_node(dt, 1, [2, 5, 3, 3], c, out_dims=[2, 5, 3, 4]) == 0 and bh.ask_node(dt, 15, [2, 5, 3, 3], out_dims=[2, 5, 9]) == 0
        assert bh.ask_node(dt, 1, [2, 5, 3, 3], c, with_param=False) == 0 and bh.ask_node(dt, 15, [2, 5, 3, 3], x_const=True) == 0
        for name in ("data", "out"):
            for typ, const in ((1, c), (15, None)):
                g = bh.node_graph(dt, typ, (2, 5, 3, 3), (0.05, 0), (0.05, 0), const)
                t = [t for t in g.tensors if t.name == name][0]
                t.scales, t.zero_points = [t.scales[0]] * 5, [t.zero_points[0]] * 5
                assert "per-tensor quant params on both sides" in bh.library_error(tm2.write_tm2(g)), (name, typ)
        g = bh.node_graph(dt, 1, (2, 5, 3, 3), (0.05, 0), (0.05, 0), c)
        t = [t for t in g.tensors if t.name == "scalar"][0]
        t.scales, t.zero_points = [t.scales[0]] * 2, [0, 0]
        assert "needs one (scale, zero point) pair" in bh.library_error(tm2.write_tm2(g))
    assert bh.ask_node(DT_FP32, 1, [2, 5, 3, 3], ("f32", 0.5)) == 0 and bh.ask_node(DT_FP32, 15, [2, 5, 3, 3]) == 0
    for typ, const in ((1, ("f32", 0.5)), (15, None)):
        assert "int8 and uint8 graphs only" in bh.library_error(tm2.write_tm2(bh.node_graph(DT_FP32, typ, (2, 5, 3, 3), None, None, const)))
    # a constant of the activation's own shape, and a constant gate, stay refused
    assert sh.ask_node(DT_UINT8, 2, [2, 5, 3, 3], [2, 5, 3, 3], b_const=True) == 0 and sh.ask_node(DT_UINT8, 0, [2, 5, 3, 3], [2, 5, 1, 1], b_const=True) == 0


def test_codes_and_answers_of_the_other_operators():
    """the op-support vectors of tests/test_crop_cpu.py hold for codes 0 .. 30 in the three graph types; 31 is a reserved, never-supported
    code like 21, 24, 27 and 29; 32 is BatchNorm, uint8 alone (no operator before this change: the last line fails on the parent)"""
    L = capi.lib()
    FP16 = 1
    assert [L.tamd_op_supported(op, DT_INT8) for op in range(31)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 0]
    assert [L.tamd_op_supported(op, DT_UINT8) for op in range(31)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 1]
    assert [L.tamd_op_supported(op, DT_FP32) for op in range(31)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1] + [0] * 15
    assert [L.tamd_op_supported(31, dt) for dt in (DT_FP32, FP16, DT_INT8, DT_UINT8)] == [0, 0, 0, 0]
    assert [L.tamd_op_supported(32, dt) for dt in (DT_FP32, FP16, DT_INT8, DT_UINT8)] == [0, 0, 0, 1]
    assert [L.tamd_op_supported(33, dt) for dt in (DT_FP32, FP16, DT_INT8, DT_UINT8)] == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_tmfile_round_trip_of_a_one_input_eltwise(ref, dtype):
    """tm2.write_tm2 writes a one-input Eltwise with shift / power / scale the way the reference's loader reads them; read_tm2 gives them
    back; the library infers the input's shape for the output whatever the file says"""
    params = {"shift": 1.5, "scale": 0.5, "power": 3.0}
    g = bh.node_graph(dtype, 17, (1, 4, 8, 8), (0.05, 0), (0.05, 0), None, params)
    b = tm2.write_tm2(g)
    node = [n for n in tm2.read_tm2(b).nodes if n.op == "Eltwise"]
    assert len(node) == 1 and len(node[0].inputs) == 1 and node[0].params == dict(params, type=17, caffe_flavor=1)
    out = ref.run_model(b, bh.all_bytes(dtype), lh.ref_mode(ref, dtype))
    assert len(out) == 1 and out[0].shape == (1, 4, 8, 8) and out[0].dtype == lh.NP[dtype]
    [t for t in g.tensors if t.name == "out"][0].dims = [1, 4, 64]
    assert bh.library_output_shape(tm2.write_tm2(g))[0] == (1, 4, 8, 8)


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("build,ops", [(bh.normalise_graph, ["Convolution"] * 2 + ["Eltwise"] * 2), (bh.hardswish_graph, ["Clip"] + ["Convolution"] * 2 + ["Eltwise"] * 3),
                                       (bh.unary_chain_graph, ["Convolution"] * 2 + ["Eltwise"] * 2)], ids=["normalise", "hardswish", "unary"])
def test_plugin_keeps_the_graph_in_one_hip_subgraph(ref, build, ops, dtype):
    """the split happens before the device is touched: input normalisation in front of a convolution, the HardSwish decomposition between
    two convolutions and unary nodes between two are each ONE "HIP" subgraph (the Eltwise nodes were CPU nodes before)"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = build(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and sorted(real[0][1]) == ops, real


def test_plugin_leaves_what_is_refused_to_the_cpu_device(ref):
    """an int8 graph with an fp32 constant, a uint8 RSQRT whose zero-point byte is 0.0, and the fp32 forms: the Eltwise stays a CPU node"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = bh.Chain(51, DT_INT8, (1, 8, 6, 6))
    x = c.conv(8, 3, 1)
    cst = bh.const_of(c.g, "half", ("f32", 0.5))
    y = c._var("scaled", c.dims(x), (c.scale(x) * 0.5, 0))
    c.last = c.g.add_node("scaled", "Eltwise", [x, cst], [y], type=1, caffe_flavor=1)
    c.cur = y
    c.conv(6, 1)
    g, xin = c.done()
    real = _real(tp._split_only(ref, g, xin, ref.MODE_INT8))
    assert [o for dev, os_ in real if dev != "HIP" for o in os_] == ["Eltwise"] and len([1 for dev, _ in real if dev == "HIP"]) == 2, real
    c = bh.Chain(52, DT_UINT8, (1, 8, 6, 6))
    c.conv(8, 3, 1); c.unary(7, (0.05, 0)); c.conv(6, 1)
    g, xin = c.done()
    real = _real(tp._split_only(ref, g, xin, ref.MODE_UINT8))
    assert [o for dev, os_ in real if dev != "HIP" for o in os_] == ["Eltwise"], real


def test_table_builders_alone_under_the_sanitizers(tmp_path):
    """tests/csrc/eltwise_tables_check.cc + csrc/lut_tables.cc and nothing else, built with -fsanitize=address,undefined: every parameter
    set's table is built, every refusal is walked, the program exits 0, and its tables and pair checksums are the library's (another
    compiler, the same bytes); the BatchNorm's per-channel table and what it refuses as not finite are walked there too"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "eltwise_tables_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "csrc", "eltwise_tables_check.cc"), os.path.join(ROOT, "tengine_amd", "csrc", "lut_tables.cc"),
                           "-lm", "-o", exe])
    hexf = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]
    args = []
    for _, typ, dtype, in_q, out_q, const, params in bh.PARAM_SETS:
        p = params or {}
        args += [str(typ), str(dtype), hexf(in_q[0]), str(in_q[1]), hexf(out_q[0]), str(out_q[1]), hexf(bh.const_value(const) if const is not None else 0.0),
                 hexf(p.get("shift", 0.0)), hexf(p.get("power", 1.0)), hexf(p.get("scale", 1.0))]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(bh.PARAM_SETS) + 9 and lines[-1].startswith("batchnorm ")
    bn_line = lines.pop()
    for line, s in zip(lines, bh.PARAM_SETS):
        assert np.array_equal(np.frombuffer(bytes.fromhex(line), np.uint8), bh.table_of(*s[1:])[1]), s[0]
    L = capi.lib()
    for line in lines[len(bh.PARAM_SETS):]:
        _, dt, typ, want = line.split()
        dt, typ = int(dt), int(typ)
        z = (lambda v: v) if dt == DT_UINT8 else (lambda v: 0)
        total = 0
        for a in range(256):
            for b in range(256):
                total = (total * 31 + L.tamd_eltwise_pair(typ, dt, a, 0.05, z(100), b, 0.02, z(140), 0.05, z(128))) % (1 << 64)
        assert total == int(want), (dt, typ)
    total = 0
    for caffe in range(2):
        for k in range(16):
            f = lambda v: float(np.float32(v))
            gamma = f(np.float32(-1.0 if k % 2 else 1.0) * (np.float32(0.2) + np.float32(0.11) * np.float32(k)))
            beta, mean = f(np.float32(0.4) * np.float32(k - 8)), f(np.float32(0.1) * np.float32(k - 5))
            var = f(np.float32(0.3) * np.float32(k)) if k % 5 else f(1e-7)
            rc, t = capi.batchnorm_table(gamma, beta, mean, var, f(0.05), 128, f(0.04), 120, 1.0 if k % 3 else 0.0, f(2e-5) if k % 2 else f(1e-3), caffe)
            assert rc == 0
            for v in t:
                total = (total * 31 + int(v)) % (1 << 64)
    assert total == int(bn_line.split()[1])


# ---- byte-pure chains as one table (tamd_graph_bytemap_chain: what the planners ask, before their own layout conditions) ----

def _ops(g, members):
    return [(g.nodes[i].op, g.nodes[i].params.get("type")) for i in members]


CHAINS = [
    ("silu", lambda dt: bh.silu_graph(dt), [("Sigmoid", None), ("Eltwise", 0)]),
    ("hardswish", lambda dt: bh.hardswish_graph(dt), [("Eltwise", 2), ("Clip", None), ("Eltwise", 0), ("Eltwise", 1)]),
    ("normalise", lambda dt: bh.normalise_graph(dt), [("Eltwise", 5), ("Eltwise", 1)]),
    ("unary", lambda dt: bh.unary_chain_graph(dt), [("Eltwise", 15), ("Eltwise", 14)]),
    ("two_branches", lambda dt: bh.two_branch_graph(dt), [("Clip", None), ("Sigmoid", None), ("Eltwise", 0)]),
    ("branch_beside_a_chain", lambda dt: bh.two_branch_graph(dt, side_reader=True), [("Clip", None), ("Eltwise", 15)]),
]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("row", CHAINS, ids=[r[0] for r in CHAINS])
def test_chain_table_is_the_node_tables_composed(row, dtype):
    """the members are the expected nodes, and the one table equals table_k[.. table_1[b]] / tamd_eltwise_pair(val_a[b], val_b[b]) built
    node by node in Python from the single-node builders -- which test_table_is_the_reference_on_every_byte and
    test_pair_is_the_reference_on_every_byte_pair hold to the reference"""
    _, build, want = row
    g, _ = build(dtype)
    members, table = capi.bytemap_chain(tm2.write_tm2(g), bh.chain_start(g))
    assert _ops(g, members) == want
    assert np.array_equal(table, bh.compose(g, members))
    assert len(np.unique(table)) > 8                          # (not a constant map: the chain's ranges are live)


def test_uint8_hardswish_with_a_division_is_one_chain():
    g, _ = bh.hardswish_graph(DT_UINT8, div=True)
    members, table = capi.bytemap_chain(tm2.write_tm2(g), bh.chain_start(g))
    assert _ops(g, members) == [("Eltwise", 2), ("Clip", None), ("Eltwise", 0), ("Eltwise", 10)] and np.array_equal(table, bh.compose(g, members))


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_chain_guards(dtype, monkeypatch):
    """an intermediate that is a graph output, or that has a reader outside the set, ends the set there; a single table node is no
    chain; a same-shape Eltwise does not start one; TAMD_PIN=bytemap_chain=0 finds none"""
    g, _ = bh.silu_graph(dtype, sigmoid_is_output=True)
    assert capi.bytemap_chain(tm2.write_tm2(g), bh.chain_start(g)) == ([], None)
    g, _ = bh.hardswish_second_reader_graph(dtype)
    b = tm2.write_tm2(g)
    members, table = capi.bytemap_chain(b, bh.chain_start(g))
    assert _ops(g, members) == [("Eltwise", 2), ("Clip", None)] and np.array_equal(table, bh.compose(g, members))
    prod = [i for i, n in enumerate(g.nodes) if n.op == "Eltwise" and n.params["type"] == 0][0]
    scal = [i for i, n in enumerate(g.nodes) if n.op == "Eltwise" and n.params["type"] == 1][0]
    clip = [i for i, n in enumerate(g.nodes) if n.op == "Clip"][0]
    conv = [i for i, n in enumerate(g.nodes) if n.op == "Convolution"][0]
    for i in (prod, scal, clip, conv):
        assert capi.bytemap_chain(b, i) == ([], None), i
    g, _ = bh.silu_graph(dtype)
    b = tm2.write_tm2(g)
    assert len(capi.bytemap_chain(b, bh.chain_start(g))[0]) == 2
    monkeypatch.setenv("TAMD_PIN", "bytemap_chain=0")
    assert capi.bytemap_chain(b, bh.chain_start(g)) == ([], None)


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_keeps_conv_silu_conv_in_one_hip_subgraph(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = bh.silu_graph(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and sorted(real[0][1]) == ["Convolution", "Convolution", "Eltwise", "Sigmoid"], real


# ---- uint8 BatchNorm: a byte map per channel (tamd_batchnorm_table) ----

@pytest.mark.parametrize("rank", [2, 3, 4])
@pytest.mark.parametrize("case", bh.BN_SETS, ids=[s[0] for s in bh.BN_SETS])
def test_batchnorm_table_is_the_reference_on_every_byte_and_channel(ref, case, rank):
    """all 256 bytes x 16 channels -- gamma and beta of mixed sign, tiny variances -- on [256, 16], [1, 16, 256] and (1, 16, 16, 16):
    rescale_factor 0, 0.5 and 1, caffe and not; the reference's CPU device twice, against tamd_batchnorm_table per channel"""
    _, iq, oq, rs, eps, caffe = case
    st = bh.bn_stats(16, 7 + rank)
    x = bh.bn_all_bytes(rank)
    assert all(np.array_equal(np.sort(np.moveaxis(x, 1, 0).reshape(16, -1)[c]), np.arange(256)) for c in range(16))
    assert (st[0] < 0).any() and (st[0] > 0).any() and (st[1] < 0).any() and (st[1] > 0).any() and (st[3] < 1e-6).any()
    b = tm2.write_tm2(bh.bn_graph(x.shape, iq, oq, st, rs, eps, caffe))
    want = ref.run_model(b, x, ref.MODE_UINT8)[0]
    assert np.array_equal(want, ref.run_model(b, x, ref.MODE_UINT8)[0]) and want.dtype == np.uint8
    got = bh.bn_apply(bh.bn_tables(16, iq, oq, st, rs, eps, caffe), x)
    assert np.array_equal(got, want.reshape(got.shape)), int((got != want.reshape(got.shape)).sum())
    assert want.min() == 0 and want.max() == 255
    assert "atch" not in bh.library_error(b)                  # validation lets the node through, as far as the device


def test_batchnorm_caffe_flavor_reads_neither_gamma_nor_beta():
    st = bh.bn_stats(4, 3)
    a = bh.bn_tables(4, (0.05, 128), (0.04, 128), st, caffe_flavor=1)
    other = (st[0] * 3 + 1, st[1] - 2, st[2], st[3])
    assert np.array_equal(a, bh.bn_tables(4, (0.05, 128), (0.04, 128), other, caffe_flavor=1))
    assert not np.array_equal(bh.bn_tables(4, (0.05, 128), (0.04, 128), st), bh.bn_tables(4, (0.05, 128), (0.04, 128), other))


BN_REFUSED = [
    ("int8", dict(dtype=DT_INT8), "the reference has no int8 kernel"),
    ("fp32", dict(dtype=DT_FP32), "uint8 graphs only"),
    ("rank_1", dict(dims=(16,)), "2-D [N,C], 3-D [N,C,W] or 4-D [N,C,H,W]"),
    ("rank_5", dict(dims=(1, 16, 2, 2, 2)), "2-D [N,C], 3-D [N,C,W] or 4-D [N,C,H,W]"),
    ("statistic_not_fp32", dict(stat_dtype=DT_UINT8), "must be fp32 constants of C elements"),
    ("statistic_of_another_length", dict(stat_len=15), "must be fp32 constants of C elements"),
    ("statistic_not_constant", dict(stat_var=True), "must be fp32 constants of C elements"),
    ("negative_variance", dict(var=-1.0), "table is not finite"),
    ("infinite_gamma", dict(gamma=float("inf")), "table is not finite"),
    ("zero_output_scale", dict(out_q=(0.0, 0)), "table is not finite"),
]


@pytest.mark.parametrize("row", BN_REFUSED, ids=[r[0] for r in BN_REFUSED])
def test_batchnorm_refusals_by_name(row):
    """prerun's validation, which runs before the device is touched, names the reason"""
    _, kw, reason = row
    kw = dict(kw)
    dims = kw.pop("dims", (2, 16, 3, 3))
    C = dims[1] if len(dims) > 1 else dims[0]
    st = [v.copy() for v in bh.bn_stats(C, 5, tiny_var=False)]
    if "var" in kw:
        st[3][2] = kw.pop("var")
    if "gamma" in kw:
        st[0][1] = kw.pop("gamma")
    out_q = kw.pop("out_q", (0.04, 128))
    dtype = kw.get("dtype", DT_UINT8)
    iq = (0.05, 0 if dtype == DT_INT8 else 128)
    err = bh.library_error(tm2.write_tm2(bh.bn_graph(dims, iq, (out_q[0], 0 if dtype == DT_INT8 else out_q[1]), st, **kw)))
    assert reason in err, err


def test_batchnorm_per_channel_parameters_and_input_count_are_refused():
    st = bh.bn_stats(16, 5)
    for name in ("data", "out"):
        g = bh.bn_graph((2, 16, 3, 3), (0.05, 128), (0.04, 128), st)
        t = [t for t in g.tensors if t.name == name][0]
        t.scales, t.zero_points = [t.scales[0]] * 16, [t.zero_points[0]] * 16
        assert "per-tensor quant params on both sides" in bh.library_error(tm2.write_tm2(g)), name
    g = bh.bn_graph((2, 16, 3, 3), (0.05, 128), (0.04, 128), st)
    n = [n for n in g.nodes if n.op == "BatchNormalization"][0]
    n.inputs = n.inputs[:3]
    assert "takes five inputs" in bh.library_error(tm2.write_tm2(g))


def test_tmfile_round_trip_of_operator_1(ref):
    """tm2.write_tm2 writes operator 1 with TM2_BatchNormParam the way the reference's loader reads it; read_tm2 gives it back; the
    library infers the input's shape for the output"""
    st = bh.bn_stats(16, 5)
    g = bh.bn_graph((2, 16, 3), (0.05, 128), (0.04, 128), st, rescale_factor=0.5, eps=0.25, caffe_flavor=1)
    b = tm2.write_tm2(g)
    node = [n for n in tm2.read_tm2(b).nodes if n.op == "BatchNormalization"]
    assert len(node) == 1 and len(node[0].inputs) == 5 and node[0].params == {"rescale_factor": 0.5, "eps": 0.25, "caffe_flavor": 1}
    out = ref.run_model(b, lh.random_bytes(3, DT_UINT8, (2, 16, 3)), ref.MODE_UINT8)
    assert len(out) == 1 and out[0].size == 96
    [t for t in g.tensors if t.name == "out"][0].dims = [2, 48]
    assert bh.library_output_shape(tm2.write_tm2(g))[0] == (2, 16, 3)


@pytest.mark.parametrize("n", [1, 2])
def test_plugin_keeps_mobilefacenets_two_ends_in_one_hip_subgraph(ref, n):
    """SUB_SCALAR -> PROD_SCALAR -> conv s2 -> PReLU -> bottleneck + SUM -> conv -> PReLU -> depthwise 7x7 -> FullyConnected -> BatchNorm:
    every operator of mobilefacenets_benchmark.tmfile, ONE "HIP" subgraph in a uint8 graph (the split happens before the device is
    touched)"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = bh.mobilefacenet_ends_graph(n)
    assert sorted({nd.op for nd in g.nodes} - {"InputOp", "Const"}) == ["BatchNormalization", "Convolution", "Eltwise", "FullyConnected", "PReLU"]
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert len(real) == 1 and real[0][0] == "HIP" and len(real[0][1]) == 15, real


def test_plugin_leaves_the_int8_batchnorm_to_the_cpu_device(ref):
    """the reference has no int8 kernel: the node stays a CPU node, by name, behind a "HIP" convolution"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = bh.Chain(53, DT_INT8, (1, 8, 6, 6))
    x = c.conv(16, 3, 1)
    st = bh.bn_stats(16, 5)
    ins = [x] + [c.g.add_const(name, v, DT_FP32) for name, v in zip(("gamma", "beta", "mean", "var"), st)]
    y = c._var("bn", c.dims(x), (c.scale(x), 0))
    c.last = c.g.add_node("bn", "BatchNormalization", ins, [y], rescale_factor=1.0, eps=1e-5, caffe_flavor=0)
    c.cur = y
    g, xin = c.done()
    pl = [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in tp._split_only(ref, g, xin, ref.MODE_INT8) if r]
    cpu = [o for dev, os_ in pl if dev != "HIP" for o in os_]
    assert len(cpu) == 1 and cpu[0].lower().startswith("batchnorm") and [os_ for dev, os_ in pl if dev == "HIP"] == [["Convolution"]], pl
