"""The channel-gate Eltwise of a Squeeze-and-Excitation block -- x (N, C, H, W) op gate (N, C, 1, 1) -- the parts that need no GPU: the
numpy restatement against the real reference library on all 65 536 byte pairs, the committed golden against the reference, what the
support query answers and what prerun refuses (each form by its own name), what the reference itself does with a gate listed first,
shape inference, and where the plugin's splitter puts the node."""
import os

import numpy as np
import pytest

import lut_helpers as lh
import se_helpers as sh
from tengine_amd import tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, ELT_MAX, ELT_PROD, ELT_SUB, ELT_SUM

PAIRS = [(dt, typ) for dt in (DT_INT8, DT_UINT8) for typ in sh.TYPES]
PAIR_IDS = ["%s_%s" % ("i8" if dt == DT_INT8 else "u8", typ) for dt, typ in PAIRS]


@pytest.mark.parametrize("dtype,typ", PAIRS, ids=PAIR_IDS)
def test_restatement_is_the_reference_on_every_byte_pair(ref, dtype, typ):
    """x (1, 256, 16, 16) with every channel holding all 256 values against gate byte c in channel c: all 65 536 pairs, and both ends of
    the clamp are reached"""
    g, xs = sh.all_pairs_case(dtype, typ)
    want = sh.reference_outputs(ref, g, xs, dtype)[0]
    again = sh.reference_outputs(ref, g, xs, dtype)[0]
    qx, qg, qo = sh.QUANT[dtype]
    got = sh.restate(dtype, typ, xs[0], xs[1], qx, qg, qo[typ])
    assert want.shape == (1, 256, 16, 16) and want.dtype == lh.NP[dtype] and np.array_equal(want, again)
    assert np.array_equal(got, want), int((got != want).sum())
    lo, hi = (-127, 127) if dtype == DT_INT8 else (0, 255)
    assert want.min() == lo and want.max() == hi and (want == lo).sum() > 1 and (want == hi).sum() > 1
    xb, gb = xs[0].view(np.uint8).reshape(256, 256), xs[1].view(np.uint8).reshape(256)
    assert all(np.array_equal(np.sort(xb[c]), np.arange(256)) for c in range(256)) and np.array_equal(gb, np.arange(256))      # every pair, once


@pytest.mark.parametrize("dims", [(1, 5, 3, 3), (2, 5, 3, 3), (2, 20, 7, 7)], ids=lambda d: "x".join(map(str, d)))
def test_restatement_is_the_reference_on_random_bytes_at_batch_2(ref, dims):
    for dtype in (DT_INT8, DT_UINT8):
        for typ in sh.TYPES:
            g, xs = sh.geometry_case(dtype, typ, dims, 31)
            qx, qg, qo = sh.QUANT[dtype]
            assert np.array_equal(sh.reference_outputs(ref, g, xs, dtype)[0], sh.restate(dtype, typ, xs[0], xs[1], qx, qg, qo[typ])), (dtype, typ)


def test_golden_is_the_real_reference(ref):
    """tests/golden/se_cases.npz (tools/make_golden_se.py) holds the inputs of every GPU case and what the reference computes from them"""
    z = sh.golden()
    cases = sh.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    assert os.path.getsize(sh.GOLDEN) < 128 * 1024
    for case in sorted(stored):
        dtype, build = cases[case]
        g, xs = build()
        assert int(z[case + "__nin"]) == len(xs)
        for i, x in enumerate(xs):
            assert z["%s__in%d" % (case, i)].dtype == x.dtype and np.array_equal(z["%s__in%d" % (case, i)], x), case
        want = sh.reference_outputs(ref, g, xs, dtype)
        assert sh.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not sh.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = sh.gpu_cases()
    for c in (5, 16, 20):
        _, xs = cases["i8_lanes_c%d" % c][1]()
        assert xs[0].shape == (2, c, 3, 3) and xs[1].shape == (2, c, 1, 1) and (xs[0] == -128).any() and (xs[1] == -128).any()
        assert not np.array_equal(xs[1][0], xs[1][1])                   # a gate indexed without n shows
    g, xs = cases["u8_planes_49_bytes_batch2"][1]()
    assert xs[0].shape[2] * xs[0].shape[3] == 49 and xs[0].shape[0] == 2
    g, xs = cases["u8_planes_335_bytes"][1]()
    assert xs[0].shape[2] * xs[0].shape[3] == 335 and xs[0].shape[1] == 2
    for k in ("i8_se_block", "u8_se_block"):
        g, xs = cases[k][1]()
        assert [n.op for n in g.nodes if n.op not in ("InputOp", "Const")] == ["Convolution", "Pooling", "Convolution", "ReLU", "Convolution", "Sigmoid", "Eltwise", "Convolution"]
        assert xs[0].shape == (2, 8, 6, 6)
    g, _ = cases["i8_gate_first_sub"][1]()
    e = [n for n in g.nodes if n.op == "Eltwise"][0]
    assert g.tensors[e.inputs[0]].dims == [1, 5, 1, 1] and g.tensors[e.inputs[1]].dims == [1, 5, 3, 3] and e.params["type"] == ELT_SUB
    g, _ = cases["u8_multi_reader"][1]()
    assert len(g.output_nodes) == 2 and sorted(g.nodes[n].op for n in g.output_nodes) == ["Eltwise", "Sigmoid"]


def test_support_query_accepts_the_gate_forms():
    """tamd_node_supported answers 1 for the channel gate in int8 and uint8 graphs (0 before the feature existed)"""
    for dt in (DT_INT8, DT_UINT8):
        for typ in (ELT_PROD, ELT_SUM, ELT_SUB):
            assert sh.ask_node(dt, typ, [2, 5, 3, 3], [2, 5, 1, 1]) == 1, (dt, typ)
            assert sh.ask_node(dt, typ, [1, 256, 16, 16], [1, 256, 1, 1]) == 1
            assert sh.ask_node(dt, typ, [1, 5, 1, 1], [1, 5, 3, 3]) == 1            # the gate listed first, batch 1
            assert sh.ask_node(dt, typ, [1, 16, 1, 2], [1, 16, 1, 1]) == 1
    # the same-shape form keeps its answers, fp32 included
    for dt in (DT_INT8, DT_UINT8, DT_FP32):
        for typ in (ELT_PROD, ELT_SUM, ELT_SUB, ELT_MAX):
            assert sh.ask_node(dt, typ, [2, 5, 3, 3], [2, 5, 3, 3]) == 1
        assert sh.ask_node(dt, 1, [2, 5, 3, 3], [2, 5, 3, 3]) == 0 and sh.ask_node(dt, 9, [2, 5, 3, 3], [2, 5, 3, 3]) == 0
        assert sh.ask_node(dt, ELT_SUM, [2, 5, 3, 3], [2, 5, 3, 3], b_const=True) == 0
        assert sh.ask_node(dt, ELT_SUM, [2, 5, 3, 3], [2, 5, 3, 3], with_param=False) == 0


# (what it is, type, x dims, small dims, gate first, part of the reason prerun's validation gives)
REFUSED = [
    ("max_with_a_gate", ELT_MAX, (2, 5, 3, 3), (2, 5, 1, 1), False, "MAX has no channel-gate form"),
    ("gate_first_batch_2", ELT_PROD, (2, 5, 3, 3), (2, 5, 1, 1), True, "listed first is defined for batch 1 only"),
    ("gate_first_batch_2_sum", ELT_SUM, (2, 5, 3, 3), (2, 5, 1, 1), True, "listed first is defined for batch 1 only"),
    ("gate_2d", ELT_PROD, (2, 5, 3, 3), (2, 5), False, "dims exactly (N, C, 1, 1)"),
    ("gate_batch_in_channels", ELT_PROD, (2, 5, 3, 3), (1, 10, 1, 1), False, "dims exactly (N, C, 1, 1)"),
    ("gate_3d", ELT_SUM, (1, 5, 3, 3), (5, 1, 1), False, "dims exactly (N, C, 1, 1)"),
    ("one_element", ELT_SUM, (2, 5, 3, 3), (1, 1, 1, 1), False, "one-element operand"),
    ("one_element_1d", ELT_SUB, (2, 5, 3, 3), (1,), False, "one-element operand"),
    ("row_form", ELT_SUM, (1, 4, 3, 3), (1, 1, 3, 3), False, "row form"),
    ("row_form_1d", ELT_SUM, (1, 4, 3, 3), (9,), False, "row form"),
    ("another_count", ELT_PROD, (2, 5, 3, 3), (1, 5, 1, 1), False, "must be a channel gate (N, C, 1, 1)"),
    ("x_3d", ELT_PROD, (5, 3, 3), (5, 1, 1), False, "must be 4-D (N, C, H, W)"),
    ("scalar_type", 1, (2, 5, 3, 3), (2, 5, 1, 1), False, "scalar and unary"),
    ("scalar_type_sum", 3, (2, 5, 3, 3), (1, 1, 1, 1), False, "scalar and unary"),
    ("unary_type", 9, (2, 5, 3, 3), (2, 5, 1, 1), False, "scalar and unary"),
]


@pytest.mark.parametrize("row", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_forms_are_refused_by_name(row):
    """tamd_node_supported answers 0, and prerun's validation (which runs before the device is touched) names the reason"""
    _, typ, xd, gd, first, reason = row
    for dt in (DT_INT8, DT_UINT8):
        a, b = (gd, xd) if first else (xd, gd)
        assert sh.ask_node(dt, typ, list(a), list(b)) == 0
        err = sh.library_error(tm2.write_tm2(sh.gate_graph(dt, typ, xd, gd, gate_first=first)))
        assert reason in err, err


def test_refused_quantisation_constants_and_fp32():
    for dt in (DT_INT8, DT_UINT8):
        assert sh.ask_node(dt, ELT_PROD, [2, 5, 3, 3], [2, 5, 1, 1], b_const=True) == 0
        assert sh.ask_node(dt, ELT_PROD, [2, 5, 3, 3], [2, 5, 1, 1], a_quant=5) == 0
        assert sh.ask_node(dt, ELT_PROD, [2, 5, 3, 3], [2, 5, 1, 1], b_quant=5) == 0
        assert sh.ask_node(dt, ELT_PROD, [2, 5, 3, 3], [2, 5, 1, 1], out_quant=5) == 0
        assert sh.ask_node(dt, ELT_PROD, [2, 5, 3, 3], [2, 5, 1, 1], out_dims=[2, 5, 1, 1]) == 0
        assert "neither operand may be a constant" in sh.library_error(tm2.write_tm2(sh.gate_graph(dt, "prod", (2, 5, 3, 3), (2, 5, 1, 1), const_gate=True)))
        for name in ("data", "gate", "out"):
            g = sh.gate_graph(dt, "prod", (2, 5, 3, 3), (2, 5, 1, 1))
            t = [t for t in g.tensors if t.name == name][0]
            t.scales, t.zero_points = [t.scales[0]] * 5, [t.zero_points[0]] * 5
            assert "per-tensor quant params on all three tensors" in sh.library_error(tm2.write_tm2(g)), name
    assert sh.ask_node(DT_FP32, ELT_PROD, [2, 5, 3, 3], [2, 5, 1, 1]) == 0
    assert "int8 and uint8 graphs only" in sh.library_error(tm2.write_tm2(sh.gate_graph(DT_FP32, "prod", (2, 5, 3, 3), (2, 5, 1, 1))))
    # .. and what runs is not refused: validation passes, and prerun gets as far as the device (or through, where there is one)
    for first in (False, True):
        ok = sh.library_error(tm2.write_tm2(sh.gate_graph(DT_INT8, "sub", (1, 5, 3, 3), (1, 5, 1, 1), gate_first=first)))
        assert "Eltwise" not in ok and "eltwise" not in ok, ok


@pytest.mark.parametrize("typ", ["prod", "sub"])
def test_reference_fails_on_a_gate_listed_first_at_batch_2(ref, typ):
    """the swapped path of eltwise_ref.c takes input_chan = dims[1] (C, not N * C): no branch fits, run_graph fails -- there are no
    bytes to equal, which is why the device refuses the form"""
    for dtype in (DT_INT8, DT_UINT8):
        g, xs = sh.geometry_case(dtype, typ, (2, 5, 3, 3), 3, gate_first=True)
        with pytest.raises(RuntimeError, match="run_graph failed"):
            sh.reference_outputs(ref, g, xs, dtype)


def test_gate_listed_first_at_batch_1_is_x_op_gate_in_the_reference(ref):
    """.. for SUB too: x - gate, although the node lists the gate first; the output has x's dims"""
    for dtype in (DT_INT8, DT_UINT8):
        qx, qg, qo = sh.QUANT[dtype]
        for typ in sh.TYPES:
            g, xs = sh.geometry_case(dtype, typ, (1, 5, 3, 3), 7, gate_first=True)
            out = sh.reference_outputs(ref, g, xs, dtype)[0]
            assert out.shape == (1, 5, 3, 3) and np.array_equal(out, sh.restate(dtype, typ, xs[0], xs[1], qx, qg, qo[typ])), (dtype, typ)


def test_shape_inference_of_a_gate_listed_first_gives_the_big_operands_dims():
    for dtype in (DT_INT8, DT_UINT8):
        g = sh.gate_graph(dtype, "prod", (1, 5, 3, 4), (1, 5, 1, 1), gate_first=True)
        [t for t in g.tensors if t.name == "out"][0].dims = [1, 5, 1, 1]       # what the file says is not what counts
        assert sh.library_output_shape(tm2.write_tm2(g))[0] == (1, 5, 3, 4)
        g = sh.gate_graph(dtype, "prod", (2, 5, 3, 4), (2, 5, 1, 1))
        assert sh.library_output_shape(tm2.write_tm2(g))[0] == (2, 5, 3, 4)


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_keeps_the_quantised_se_block_in_one_hip_subgraph(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = sh.se_block_graph(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP", real
    assert sorted(real[0][1]) == ["Convolution"] * 4 + ["Eltwise", "Pooling", "ReLU", "Sigmoid"], real


def test_plugin_leaves_the_fp32_gate_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = sh.se_block_graph(DT_FP32)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    on_hip = {o for dev, os_ in real if dev == "HIP" for o in os_}
    on_cpu = [o for dev, os_ in real if dev != "HIP" for o in os_]
    assert "Eltwise" not in on_hip and on_cpu.count("Eltwise") == 1 and "Convolution" in on_hip, real


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_leaves_a_max_gate_to_the_cpu_device(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = sh.se_block_graph(dtype, typ="max")
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert [o for dev, os_ in real if dev != "HIP" for o in os_] == ["Eltwise"], real
    assert len([1 for dev, _ in real if dev == "HIP"]) == 2, real
