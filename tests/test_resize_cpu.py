"""Quantised nearest Resize on the device, the parts that need no GPU: the operator codes, the tmfile writer and the library's reader
(the loader's scale swap included), the byte map on all 256 bytes and the index vectors against what the real reference computes, shape
inference against the reference's, resize_refusal's answers (each refusal by its name), the committed golden against the reference, and
where the plugin's splitter puts the node."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lut_helpers as lh
import resize_helpers as rh
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3
X = (1, 8, 3, 5)
S = rh.scales

# (id, type, (in scale, in zp), (out scale, out zp)): what each pair is for is in its id
TABLE_SETS = [
    ("i8_scales_differ", DT_INT8, (0.05, 0), (0.031, 0)),
    ("i8_equal", DT_INT8, (0.05, 0), (0.05, 0)),
    ("i8_coarser", DT_INT8, (0.02, 0), (0.07, 0)),
    ("i8_saturates_both_ends", DT_INT8, (0.2, 0), (0.05, 0)),
    ("i8_tiny_to_large", DT_INT8, (0.001, 0), (0.5, 0)),
    ("i8_ratio_3", DT_INT8, (0.03, 0), (0.01, 0)),
    ("i8_half_steps", DT_INT8, (0.05, 0), (0.1, 0)),
    ("i8_near_equal", DT_INT8, (0.0501, 0), (0.05, 0)),
    ("u8_zp0", DT_UINT8, (0.05, 0), (0.031, 12)),
    ("u8_zp77", DT_UINT8, (0.05, 77), (0.031, 12)),
    ("u8_zp255", DT_UINT8, (0.05, 255), (0.04, 200)),
    ("u8_equal", DT_UINT8, (0.05, 77), (0.05, 77)),
    ("u8_equal_zp0", DT_UINT8, (0.02, 0), (0.02, 0)),
    ("u8_saturates_both_ends", DT_UINT8, (0.2, 128), (0.05, 128)),
    ("u8_half_steps", DT_UINT8, (0.05, 100), (0.1, 100)),
    ("u8_coarser", DT_UINT8, (0.02, 128), (0.07, 3)),
]
SCALES = [(1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (4.0, 4.0), (0.5, 0.5), (1.5, 1.5), (2.5, 2.5), (1.0 / 3.0, 1.0 / 3.0), (0.7, 0.7),
          (2.0, 3.0), (3.0, 1.0), (1.5, 2.5), (0.5, 2.0), (0.7, 4.0)]
EXTENTS = range(2, 41)


def _table(case):
    _, dtype, in_q, out_q = case
    return capi.resize_table(dtype, lh.f32(in_q[0]), in_q[1], lh.f32(out_q[0]), out_q[1])


def _error(g):
    return rh.library_outcome(tm2.write_tm2(g))[1]


def test_operator_codes():
    """fails without the feature: code 36 is nobody's"""
    L = capi.lib()
    assert rh.OP_RESIZE == capi.OP_RESIZE == 36
    assert [L.tamd_op_supported(36, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 1, 1]
    assert [L.tamd_op_supported(35, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]
    assert [L.tamd_op_supported(37, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]


def test_writer_and_library_reader_round_trip_operator_54():
    """fails without the feature: the library's reader does not know tm2 operator 54 and the file cannot be loaded"""
    assert tm2.OPTYPE["Resize"] == 54
    p = {"scale_x": lh.f32(1.5), "scale_y": lh.f32(0.6), "type": 1}
    g = rh.unary_graph(DT_UINT8, (1, 4, 7, 10), (0.05, 0), (0.031, 0), p)
    b = tm2.write_tm2(g)
    node = [n for n in tm2.read_tm2(b).nodes if n.op == "Resize"]
    assert len(node) == 1 and node[0].params == p and len(node[0].inputs) == 1       # the file's three fields as they are, type included
    L = capi.lib()
    h = L.tamd_graph_load_tm2(b, len(b))
    assert h, L.tamd_last_error()
    L.tamd_graph_destroy(h)
    g.nodes[g.output_nodes[0]].params = {}                   # the defaults are resize.c's init_op: 1, 1, nearest
    assert [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "Resize"][0].params == {"scale_x": 1.0, "scale_y": 1.0, "type": 0}


def test_a_file_never_carries_bilinear(ref):
    """the reference's loader does not read `type`: a file that says 1 runs nearest there, and loads here as nearest too"""
    g, x = rh.single(DT_UINT8, (1, 3, 4, 6), S(2.0, type_=1), 5)
    b = tm2.write_tm2(g)
    g0, _ = rh.single(DT_UINT8, (1, 3, 4, 6), S(2.0), 5)
    assert np.array_equal(ref.run_model(b, x, ref.MODE_UINT8)[0], ref.run_model(tm2.write_tm2(g0), x, ref.MODE_UINT8)[0])
    shape, err = rh.library_outcome(b)
    assert shape == (1, 3, 8, 12) and "resize" not in err.lower(), (shape, err)


def test_models_builder_writes_the_node():
    b = models._B("neck", [1, 8, 5, 7])
    y = b.resize("up", b.cur, 2.0, 3.0)
    assert b.dims(y) == [1, 8, 10, 21]
    assert b.g.nodes[-1].op == "Resize" and b.g.nodes[-1].params == {"scale_x": 2.0, "scale_y": 3.0, "type": 0}
    assert b.dims(b.resize("up2", y)) == [1, 8, 20, 42]
    with pytest.raises(AssertionError):
        b.resize("bad", y, 0.0)


@pytest.mark.parametrize("case", TABLE_SETS, ids=[s[0] for s in TABLE_SETS])
def test_table_is_the_reference_on_every_byte(ref, case):
    """a x1 Resize over a tensor that holds all 256 byte values, in the reference, against tamd_resize_table: byte equality"""
    _, dtype, in_q, out_q = case
    b = tm2.write_tm2(rh.unary_graph(dtype, (1, 16, 4, 4), in_q, out_q, S(1.0)))
    want = ref.run_model(b, lh.all_bytes(dtype), lh.ref_mode(ref, dtype))[0]
    got = _table(case)
    assert got is not None and got.shape == (256,)
    assert np.array_equal(got, want.reshape(-1).view(np.uint8)), np.nonzero(got != want.reshape(-1).view(np.uint8))[0]
    # .. and it is tamd_interp_table's implementation: the same bytes
    assert np.array_equal(got, capi.interp_table(dtype, lh.f32(in_q[0]), in_q[1], lh.f32(out_q[0]), out_q[1]))


def test_parameter_sets_reach_the_branches_they_are_named_for():
    sets = {s[0]: s for s in TABLE_SETS}
    assert sum(s[1] == DT_INT8 for s in TABLE_SETS) >= 8 and sum(s[1] == DT_UINT8 for s in TABLE_SETS) >= 8
    ident = np.arange(256, dtype=np.uint8)
    eq = _table(sets["i8_equal"])
    assert eq[0x80] == 0x81                                             # -128 comes out as -127: an int8 "copy" would be wrong
    assert np.array_equal(np.delete(eq, 0x80), np.delete(ident, 0x80))
    assert np.array_equal(_table(sets["u8_equal"]), ident) and np.array_equal(_table(sets["u8_equal_zp0"]), ident)
    i8 = _table(sets["i8_saturates_both_ends"]).view(np.int8)
    assert (i8 == 127).sum() > 1 and (i8 == -127).sum() > 1 and i8.min() == -127
    u8 = _table(sets["u8_saturates_both_ends"])
    assert (u8 == 255).sum() > 1 and (u8 == 0).sum() > 1
    for s in TABLE_SETS:
        if s[1] == DT_INT8:
            assert _table(s).view(np.int8).min() >= -127, s[0]          # -128 never comes out
    assert capi.resize_table(DT_FP32, 0.05, 0, 0.02, 0) is None
    # an entry the reference does not define: 0 / 0 is a NaN, x / 0 an infinity, 1e30 / 1e-30 * 127 leaves int
    assert capi.resize_table(DT_UINT8, 0.05, 0, 0.0, 0) is None and capi.resize_table(DT_INT8, 1e30, 0, 1e-8, 0) is None
    assert capi.resize_table(DT_UINT8, float("nan"), 0, 0.05, 0) is None


@pytest.mark.parametrize("sc", SCALES, ids=lambda s: "%g_%g" % s)
def test_indices_and_shape_are_the_reference_on_ramps(ref, sc):
    """extents 2 .. 40 on both axes at once: channel 0 holds the column index in every byte, channel 1 the row index, equal parameters
    (the uint8 map is the identity), so the reference's output NAMES the source column and row of every output pixel.  The shape the
    library infers from the file is the reference's, the index vectors of tamd_resize_indices are the reference's"""
    p = S(*sc)
    for n in EXTENTS:
        oh, ow = rh.out_hw(n, n, p)
        x = np.empty((1, 2, n, n), np.uint8)
        x[0, 0] = np.arange(n, dtype=np.uint8)[None, :]
        x[0, 1] = np.arange(n, dtype=np.uint8)[:, None]
        b = tm2.write_tm2(rh.unary_graph(DT_UINT8, x.shape, (0.05, 77), (0.05, 77), p))
        shape, err = rh.library_outcome(b)
        if oh < 1 or ow < 1:                                 # (2 * (1 / 3) = 0.67: the reference infers an empty tensor; refused by name)
            assert "the output is empty" in err, (n, err)
            continue
        out = ref.run_model(b, x, ref.MODE_UINT8)[0]
        assert out.shape == shape == (1, 2, oh, ow), (n, out.shape, shape, err)
        iy, ix = capi.resize_indices(n, oh, p["scale_x"]), capi.resize_indices(n, ow, p["scale_y"])
        assert iy is not None and ix is not None and iy.max() < n and ix.max() < n and iy.min() >= 0 and ix.min() >= 0
        assert np.array_equal(out[0, 0], np.repeat(ix[None, :], oh, 0)), (n, sc)
        assert np.array_equal(out[0, 1], np.repeat(iy[:, None], ow, 1)), (n, sc)
        assert np.array_equal(iy, rh.numpy_indices(n, oh, p["scale_x"])) and np.array_equal(ix, rh.numpy_indices(n, ow, p["scale_y"]))


def test_the_readers_scale_swap(ref):
    """the loader fills scale_h from scale_x and scale_w from scale_y: a file with scale_x 3, scale_y 2 triples the ROWS"""
    g, x = rh.single(DT_INT8, (1, 4, 5, 7), {"scale_x": 3.0, "scale_y": 2.0, "type": 0}, 5)
    g.tensors[g.nodes[g.output_nodes[0]].outputs[0]].dims = [1, 1, 1, 1]          # a file whose output tensor carries NO useful shape
    b = tm2.write_tm2(g)
    out = ref.run_model(b, x, ref.MODE_INT8)[0]
    shape, err = rh.library_outcome(b)
    assert out.shape == shape == (1, 4, 15, 14), (out.shape, shape, err)


def test_indices_refuse_what_the_reference_does_not_define():
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert capi.resize_indices(4, 4, bad) is None, bad
    assert capi.resize_indices(4, 0, 1.0) is None and capi.resize_indices(0, 4, 1.0) is None
    assert list(capi.resize_indices(4, 8, 2.0)) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert list(capi.resize_indices(3, 8, 2.0)) == [0, 0, 1, 1, 2, 2, 2, 2]       # the clamp: T_MIN(.., h - 1)
    assert capi.resize_indices(4, 3, 1e-30) is None                              # 1.f / scale is huge: 1 * 1e30 leaves int


# (what is asked, type, input dims, params, what else differs from a node that runs, the words of the refusal)
REFUSED = [
    ("batch_2", DT_UINT8, (2, 8, 3, 5), S(2.0), {}, "batch 1 only"),
    ("rank_3", DT_UINT8, (8, 3, 5), S(2.0), {}, "4-D tensors only"),
    ("rank_5", DT_INT8, (1, 8, 3, 5, 2), S(2.0), {}, "4-D tensors only"),
    ("constant_input", DT_UINT8, X, S(2.0), dict(data_const=True), "must not be a constant"),
    ("scale_zero", DT_INT8, X, S(0.0, 2.0), dict(out_dims=[1, 8, 1, 10]), "finite and positive"),
    ("scale_negative", DT_UINT8, X, S(2.0, -2.0), dict(out_dims=[1, 8, 6, 1]), "finite and positive"),
    ("scale_infinite", DT_UINT8, X, S(float("inf"), 2.0), dict(out_dims=[1, 8, 1, 10]), "finite and positive"),
    ("scale_nan", DT_INT8, X, S(2.0, float("nan")), dict(out_dims=[1, 8, 6, 1]), "finite and positive"),
    ("empty_output", DT_UINT8, X, S(0.25, 2.0), dict(out_dims=[1, 8, 1, 10]), "the output is empty"),
    ("extent_outside_int", DT_UINT8, X, S(2.0, 1e9), dict(out_dims=[1, 8, 6, 1]), "outside int"),
    ("per_channel_input", DT_INT8, X, S(2.0), dict(in_quant=8), "per-tensor"),
    ("per_channel_output", DT_UINT8, X, S(2.0), dict(out_quant=2), "per-tensor"),
    ("fp32", DT_FP32, X, S(2.0), {}, "int8 and uint8 graphs only"),
    ("undefined_table", DT_UINT8, X, S(2.0), dict(out_q=(0.0, 0)), "a table entry is not finite"),
]


def _refused_graph(case):
    _, dt, dims, p, kw, _ = case
    kw = dict(kw)
    return rh.unary_graph(dt, dims, rh.IN_Q.get(dt), kw.pop("out_q", rh.OUT_Q.get(dt)), p, **kw)


@pytest.mark.parametrize("case", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_forms_are_refused_by_name_when_a_file_carries_them(case):
    """through the tmfile reader and prerun's shape inference / validation, which run before the device is touched"""
    err = _error(_refused_graph(case))
    assert case[5] in err, err


def test_support_queries():
    A = rh.ask_resize
    for case, (dt, dims, p, kw) in rh.SINGLE.items():    # what runs: every single-node case of the GPU tests
        assert A(I8 if dt == DT_INT8 else U8, dims, p) == 1, case
    for name, dt, dims, p, kw, _ in REFUSED:             # .. and what does not, each as the rule says
        code = {DT_INT8: I8, DT_FP32: F32}.get(dt, U8)
        assert A(code, dims, p, out_dims=kw.get("out_dims"), const_input=kw.get("data_const", False), in_quant=kw.get("in_quant"), out_quant=kw.get("out_quant"),
                 in_q=(0.05, 0) if "out_q" in kw else None, out_q=kw.get("out_q")) == 0, name
    assert A(U8, X, S(2.0), in_q=(0.05, 3), out_q=(0.04, 7)) == 1                      # with the values: the table is checked, and defined
    assert A(I8, X, S(2.0, type_=1)) == 0 and A(U8, X, S(2.0, type_=2)) == 0           # bilinear (a graph built in memory), and no type at all
    assert A(U8, X, S(2.0), out_dims=[1, 8, 6, 11]) == 0 and A(I8, X, S(2.0), out_dims=[8, 6, 10]) == 0 and A(U8, X, S(2.0, 3.0), out_dims=[1, 8, 9, 10]) == 0
    assert A(U8, X, S(2.0, 3.0), out_dims=[1, 8, 6, 15]) == 1                          # {scale_w, scale_h}: rows by 2, columns by 3
    assert A(U8, X, S(2.0), with_param=False) == 0
    assert A(U8, X, S(2.0), inputs=2) == 0 and A(U8, X, S(2.0), inputs=0) == 0
    assert A(FP16, X, S(2.0)) == 0


def test_a_node_that_runs_gets_as_far_as_the_device():
    for case, (dt, dims, p, kw) in rh.SINGLE.items():
        g, _ = rh.single(dt, dims, p, 5, **kw)
        assert "resize" not in _error(g).lower(), case


def _hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def _rule(dt, dims, sh, sw, type_=0, has_param=1, const=0, in_quant=1, out_quant=1, q=((0.05, 77), (0.031, 12)), out=None):
    f = [dt, has_param, const, in_quant, out_quant, _hex(sh), _hex(sw), type_, _hex(q[0][0]) if q else "0", q[0][1] if q else 0, _hex(q[1][0]) if q else "0",
         q[1][1] if q else 0, len(dims)] + list(dims)
    if out is not None:
        f += [len(out)] + list(out)
    return " ".join(str(v) for v in f)


def _ok(dtype, dims, sh, sw, q=((0.05, 77), (0.031, 12)), rep=None):
    oh, ow = rh.out_hw(dims[2], dims[3], S(sh, sw))
    iy, ix = rh.numpy_indices(dims[2], oh, sh), rh.numpy_indices(dims[3], ow, sw)
    crc = 0
    if q:
        t = capi.resize_table(dtype, lh.f32(q[0][0]), q[0][1], lh.f32(q[1][0]), q[1][1])
        crc = int((t.astype(np.int64) * np.arange(1, 257)).sum())
    rep = rep or (0, 0)
    return "OK out=1,%d,%d,%d sh=%d sw=%d iy=%s ix=%s table=%d" % (dims[1], oh, ow, rep[0], rep[1], ",".join(map(str, iy)), ",".join(map(str, ix)), crc)


R = "REFUSED Resize"
# what resize_refusal answers (tests/csrc/resize_rules_check.cc): (input line, expected output line)
RULES = [
    (_rule("u8", X, 2.0, 2.0), _ok(DT_UINT8, X, 2.0, 2.0, rep=(2, 2))),
    (_rule("i8", X, 2.0, 3.0, q=((0.05, 0), (0.031, 0))), _ok(DT_INT8, X, 2.0, 3.0, q=((0.05, 0), (0.031, 0)), rep=(2, 3))),
    (_rule("u8", X, 3.0, 1.0), _ok(DT_UINT8, X, 3.0, 1.0, rep=(3, 1))),
    (_rule("u8", X, 1.0, 1.0, q=None), _ok(DT_UINT8, X, 1.0, 1.0, q=None, rep=(1, 1))),              # no quantisation values: no table
    (_rule("u8", (1, 2, 6, 10), 1.5, 2.5), _ok(DT_UINT8, (1, 2, 6, 10), 1.5, 2.5)),                 # not whole numbers: the replicate form is not legal
    (_rule("u8", (1, 2, 6, 10), 0.5, 0.5), _ok(DT_UINT8, (1, 2, 6, 10), 0.5, 0.5)),
    (_rule("u8", (1, 2, 7, 7), 0.7, 2.0), _ok(DT_UINT8, (1, 2, 7, 7), 0.7, 2.0)),                   # one axis whole, the other not: not legal
    (_rule("u8", (1, 2, 3, 40), 2.0, 1.0 / 3.0), _ok(DT_UINT8, (1, 2, 3, 40), 2.0, 1.0 / 3.0)),
    (_rule("u8", X, 2.0, 2.0, out=[1, 8, 6, 10]), _ok(DT_UINT8, X, 2.0, 2.0, rep=(2, 2))),          # the output's dims given, and right
    (_rule("u8", X, 2.0, 2.0, out=[1, 8, 6, 11]), R + ": the output does not have the dims the reference infers"),
    (_rule("u8", X, 2.0, 2.0, out=[8, 6, 10]), R + ": the output does not have the dims the reference infers"),
    (_rule("u8", X, 2.0, 2.0, has_param=0), R + " needs its parameter"),
    (_rule("f32", X, 2.0, 2.0), R + " runs on the device in int8 and uint8 graphs only"),
    (_rule("f16", X, 2.0, 2.0), R + " runs on the device in int8 and uint8 graphs only"),
    (_rule("u8", X, 2.0, 2.0, type_=1), "REFUSED only nearest Resize (type 0) runs on the device: bilinear stays on the CPU device"),
    (_rule("u8", X, 2.0, 2.0, type_=7), R + ": the type is neither nearest (0) nor bilinear (1)"),
    (_rule("u8", (8, 3, 5), 2.0, 2.0), R + " runs on the device on 4-D tensors only"),
    (_rule("i8", (1, 8, 3, 5, 2), 2.0, 2.0), R + " runs on the device on 4-D tensors only"),
    (_rule("u8", (), 2.0, 2.0), R + " runs on the device on 4-D tensors only"),
    (_rule("u8", (1, 8, 0, 5), 2.0, 2.0), R + ": every dimension must be at least 1"),
    (_rule("u8", (2, 8, 3, 5), 2.0, 2.0), R + ": the reference defines the operator for batch 1 only"),
    (_rule("u8", X, 2.0, 2.0, const=1), R + ": the input must not be a constant"),
    (_rule("u8", X, 0.0, 2.0), R + ": both scales must be finite and positive"),
    (_rule("u8", X, 2.0, -0.5), R + ": both scales must be finite and positive"),
    (_rule("u8", X, float("inf"), 2.0), R + ": both scales must be finite and positive"),
    (_rule("u8", X, 2.0, float("nan")), R + ": both scales must be finite and positive"),
    (_rule("u8", X, 2.0, 2.0, in_quant=8), R + " needs per-tensor quant params on both sides"),
    (_rule("i8", X, 2.0, 2.0, out_quant=2), R + " needs per-tensor quant params on both sides"),
    (_rule("u8", X, 2.0, 2.0, in_quant=0), R + " needs per-tensor quant params on both sides"),
    (_rule("u8", X, 2.0, 1e9), R + ": an output extent lies outside int"),                          # 5 * 1e9: the conversion is undefined
    (_rule("u8", X, 0.25, 2.0), R + ": the output is empty"),                                        # (int)(3 * 0.25) = 0
    (_rule("u8", (1, 4, 40000, 40000), 1.0, 1.0), R + ": the tensor has more than 2^31 elements"),
    (_rule("u8", (1, 64, 3000, 3000), 2.0, 2.0), R + ": the tensor has more than 2^31 elements"),    # the OUTPUT leaves 32-bit positions
    (_rule("u8", X, 2.0, 2.0, q=((0.05, 0), (1e-38, 0))), R + ": a table entry is not finite or lies outside int (the reference's conversion is undefined there)"),
    (_rule("i8", X, 2.0, 2.0, q=((float("nan"), 0), (0.05, 0))), R + ": a table entry is not finite or lies outside int (the reference's conversion is undefined there)"),
]


def test_resize_refusal_names_every_refusal_and_resolves_the_node(tmp_path):
    """the rule itself with its two builders, as a stand-alone host program (its own main, host code only) under the address and
    undefined-behaviour sanitizers: its answers are those of numpy_indices and of the library's table"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "resize_rules_check")
    csrc = os.path.join(ROOT, "tengine_amd", "csrc")
    subprocess.check_call([hipcc, "-std=c++17", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", csrc,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "csrc", "resize_rules_check.cc"), os.path.join(csrc, "resize_tables.cc"),
                           os.path.join(csrc, "interp_tables.cc"), "-o", exe], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], input="\n".join(r[0] for r in RULES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(RULES), out.stdout
    for (case, want), got in zip(RULES, lines):
        assert got == want, (case, got, want)
    assert len({w for _, w in RULES if w.startswith("REFUSED")}) >= 14           # every refusal has its own reason


def test_golden_holds_every_case_and_the_numpy_statement():
    z = rh.golden()
    cases = rh.gpu_cases()
    assert {k[:-3] for k in z.files if k.endswith("__n")} == set(cases)
    assert os.path.getsize(rh.GOLDEN) < 96 * 1024
    for case, (dt, dims, p, kw) in rh.SINGLE.items():
        g, x = cases[case][1]()
        assert np.array_equal(z[case + "__in"], x) and x.dtype == tm2.NP_OF_DT[dt], case
        iq, oq = kw.get("in_q", rh.IN_Q[dt]), kw.get("out_q", rh.OUT_Q[dt])
        want = rh.numpy_resize(x, p, capi.resize_table(dt, lh.f32(iq[0]), iq[1], lh.f32(oq[0]), oq[1]))
        assert int(z[case + "__n"]) == 1 and z[case + "__out0"].dtype == want.dtype and np.array_equal(z[case + "__out0"], want), case


def test_cases_hold_what_they_are_named_for():
    cases = rh.gpu_cases()
    g, x = cases["i8_equal_minus128"][1]()
    assert (x == -128).sum() >= 2 and (rh.golden()["i8_equal_minus128__out0"] == -128).sum() == 0
    t = lambda g, i: (g.tensors[i].scales[0], g.tensors[i].zero_points[0])
    for case, (dt, dims, p, kw) in rh.SINGLE.items():
        g, _ = cases[case][1]()
        n = g.nodes[g.output_nodes[0]]
        assert (t(g, n.inputs[0]) == t(g, n.outputs[0])) == ("identity" in case or "equal" in case), case
    assert {c for c in rh.SINGLE if "identity" in c} == {"u8_identity_x2", "u8_identity_sw3"}
    assert (3 * 2) * (5 * 2) == 60 and 60 % 16 != 0 and 5 * 2 < 16      # u8_planes_of_60: never aligned, no chunk inside a row
    assert 9 * 2 == 18 and 18 % 16 != 0                                  # u8_rows_of_18: chunks cross row boundaries, and some lie inside a row
    assert (24 * 2) % 16 == 0                                            # u8_rows_of_48: every chunk lies inside a row
    g, _ = cases["i8_source_concat_view"][1]()
    r = [n for n in g.nodes if n.op == "Resize"][0]
    cat = [n for n in g.nodes if n.op == "Concat"][0]
    assert r.inputs[0] == cat.inputs[1] and g.tensors[cat.inputs[0]].dims[1] == 16 and g.tensors[r.inputs[0]].dims[1] == 32
    for case in [c for c in cases if "into_concat" in c]:
        g, _ = cases[case][1]()
        r = [i for i, n in enumerate(g.nodes) if n.op == "Resize"][0]
        cat = [n for n in g.nodes if n.op == "Concat"][0]
        i = cat.inputs.index(g.nodes[r].outputs[0])
        assert len(cat.inputs) == 3 and i == 1, case                     # neighbours on both sides
        sides = [k for k, n in enumerate(g.nodes) if n.outputs and n.outputs[0] in (cat.inputs[0], cat.inputs[2])]
        if case.endswith("resize_last"):
            assert all(k < r for k in sides), case
        if case.endswith("resize_first"):
            assert all(k > r for k in sides), case
        for ti in cat.inputs:
            assert t(g, ti) == t(g, cat.outputs[0]), case
        if "odd_offset" in case:
            lead = g.tensors[cat.inputs[0]].dims
            assert (lead[1] * lead[2] * lead[3]) % 2 == 1, case


@pytest.mark.parametrize("case", sorted(rh.gpu_cases()))
def test_golden_is_the_real_reference(ref, case):
    """tests/golden/resize_cases.npz (tools/make_golden_resize.py) holds what the reference computes here"""
    z = rh.golden()
    dt, build = rh.gpu_cases()[case]
    g, x = build()
    assert np.array_equal(z[case + "__in"], x)
    want = rh.reference_outputs(ref, g, x, dt)
    assert rh.equals_golden(z, case, want), case
    want[0].reshape(-1)[0] ^= 1                          # .. and the comparison is one: a single changed bit is seen
    assert not rh.equals_golden(z, case, want), case


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_keeps_the_neck_block_in_one_hip_subgraph(ref, dtype):
    """fails without the feature: the plugin's operator table does not know the node and the split gives HIP / CPU / HIP"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = rh.neck_block(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert len(real) == 1 and real[0][0] == "HIP" and {rh.REF_OP_NAME, "Convolution", "Concat"} <= set(real[0][1]), real


def test_plugin_leaves_the_node_of_an_fp32_graph_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = rh.neck_block(DT_FP32)
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    nodes = [(dev, ops) for dev, ops in real if rh.REF_OP_NAME in ops]
    assert len(nodes) == 1 and nodes[0][0] != "HIP", real
    assert real[0][0] == "HIP" and "Convolution" in real[0][1] and len(real) == 3, real


def test_plugin_leaves_a_refused_form_to_the_cpu_device(ref):
    """batch 2 is not the device's (the reference moves image 0 twice and leaves the rest to chance): the node stays where the reference
    runs it, between two device subgraphs"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    k = rh.Neck(94, DT_UINT8, (2, 8, 6, 6))
    k.conv(8, 1)
    k.resize(S(2.0))
    k.conv(4, 1)
    g, x = k.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == [rh.REF_OP_NAME], real
