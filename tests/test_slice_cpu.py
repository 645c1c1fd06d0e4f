"""uint8 Slice on the device, the parts that need no GPU: the byte map (all 256 bytes) against what the reference computes, shape
inference against the reference's, every refusal by its name, the support queries, the tmfile writer and reader, where the plugin's
splitter puts the node, and the committed golden against the reference."""
import os

import numpy as np
import pytest

import lut_helpers as lh
import slice_op_helpers as so
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

F32, FP16, I8, U8 = 0, 1, 2, 3
S = so.slice_graph


def _table(case):
    _, in_q, out_q = case
    return capi.slice_table(lh.f32(in_q[0]), in_q[1], lh.f32(out_q[0]), out_q[1])


@pytest.mark.parametrize("case", so.TABLE_SETS, ids=[s[0] for s in so.TABLE_SETS])
def test_slice_table_is_the_golden_on_every_byte(case):
    """tamd_slice_table against the bytes the reference made of 0 .. 255 (a (1, 2, 16, 16) tensor through Slice(axis 1, [1, 2))), as
    the golden holds them"""
    got = _table(case)
    assert got is not None and got.shape == (256,) and got.dtype == np.uint8
    want = so.golden()["table__" + case[0]]
    assert np.array_equal(got, want), np.nonzero(got != want)[0]


@pytest.mark.parametrize("case", so.TABLE_SETS, ids=[s[0] for s in so.TABLE_SETS])
def test_slice_table_is_the_reference_on_every_byte(ref, case):
    """.. and against the reference itself, where it is built"""
    g, x = so.table_case(case[1], case[2])
    assert np.array_equal(x[0, 1].reshape(-1), np.arange(256))
    want = so.reference_outputs(ref, g, x)[0]
    assert want.shape == (1, 1, 16, 16)
    assert np.array_equal(_table(case), want.reshape(-1))


def test_parameter_sets_reach_the_branches_they_are_named_for():
    sets = {s[0]: s for s in so.TABLE_SETS}
    ident = np.arange(256, dtype=np.uint8)
    assert np.array_equal(_table(sets["equal"]), ident)
    for zp in (0, 12, 77, 128, 255):
        assert np.array_equal(capi.slice_table(lh.f32(0.05), zp, lh.f32(0.05), zp), ident), zp
    fine = _table(sets["finer_saturates_at_255"])
    assert (fine == 255).sum() > 1 and (fine == 0).sum() > 1 and fine[77] == 12
    coarse = _table(sets["coarser"])
    assert coarse[12] == 77 and 0 < coarse.min() and coarse.max() < 255 and len(set(coarse.tolist())) < 256
    assert (_table(sets["zp0_to_zp255"]) == 255).all() and (_table(sets["zp255_to_zp0"]) == 0).all()
    # (b - 3) * 0.5 + 4 with the double round(): ties away from zero -- 2.5 -> 3, 3.5 -> 4, 4.5 -> 5
    assert list(_table(sets["ties"])[:8]) == [3, 3, 4, 4, 5, 5, 6, 6]


def test_slice_table_refuses_what_the_reference_cannot_convert():
    assert capi.slice_table(0.0, 0, 0.05, 0) is None and capi.slice_table(0.05, 0, 0.0, 0) is None
    assert capi.slice_table(-0.05, 0, 0.05, 0) is None
    assert capi.slice_table(float("nan"), 0, 0.05, 0) is None and capi.slice_table(0.05, 0, float("nan"), 0) is None
    assert capi.slice_table(float("inf"), 0, 0.05, 0) is None and capi.slice_table(0.05, 0, float("inf"), 0) is None
    assert capi.slice_table(1e30, 0, 1e-8, 0) is None                   # 255e38: inf, outside int
    assert capi.slice_table(1.0, 0, 1e-8, 0) is None                    # 2.55e10: finite, outside int
    assert capi.slice_table(1.0, 0, 1e-6, 0) is not None                # 2.55e8: inside int, clamped to 255


# (id, dims, axis, begin, end, step): the rules of slice.c:116-156
SHAPES = [
    ("end_beyond", (1, 6, 3, 5), 1, 2, 100, 1),
    ("end_zero", (1, 8, 3, 5), 1, 3, 0, 1),
    ("end_negative", (1, 8, 3, 5), 1, 1, -2, 1),
    ("step2_even_extent", (1, 3, 4, 70), 3, 0, 70, 2),
    ("step2_odd_extent", (1, 3, 4, 71), 3, 0, 71, 2),
    ("step3_even_extent", (1, 2, 3, 50), 3, 0, 50, 3),
    ("step3_odd_extent", (1, 10, 3, 5), 1, 1, 10, 3),
    ("step0_means_1", (1, 8, 3, 5), 1, 2, 6, 0),
    ("negative_axis", (1, 3, 7, 5), -2, 2, 6, 1),
    ("negative_axis_w", (1, 3, 4, 37), -1, 3, 36, 1),
    ("batch_axis", (3, 4, 3, 5), 0, 1, 3, 1),
]


@pytest.mark.parametrize("case", SHAPES, ids=[s[0] for s in SHAPES])
def test_inferred_shape_is_the_references(ref, case):
    """a file whose output tensor carries NO useful shape: what the reference infers is what the library infers, and the bytes the
    reference computes are the numpy pick through the byte map"""
    _, dims, axis, begin, end, step = case
    g, x = S(dims, axis, begin, end, step, out_dims=[1, 1, 1, 1])
    b = tm2.write_tm2(g)
    out = so.reference_outputs(ref, g, x)[0]
    shape, err = so.library_outcome(b)
    assert shape == out.shape, (shape, out.shape, err)
    assert "slice" not in err.lower(), err
    pick = so.numpy_slice(x, axis % 4, begin, end, step)
    assert pick.shape == out.shape and np.array_equal(out, capi.slice_table(lh.f32(0.05), 77, lh.f32(0.031), 12)[pick])
    ax = axis % 4
    assert out.shape[ax] == so.out_extent(dims[ax], begin, end, step)


def test_full_range_is_a_raw_copy_in_the_reference(ref):
    """out dims == in dims: the input's bytes, although the two tensors' parameters differ"""
    for end in (6, 100):
        g, x = S((1, 6, 3, 5), 1, 0, end)
        assert g.tensors[0].scales != g.tensors[1].scales
        assert np.array_equal(so.reference_outputs(ref, g, x)[0], x)


def _error(g):
    return so.library_outcome(tm2.write_tm2(g))[1]


def test_refused_forms_are_refused_by_name_when_a_file_carries_them():
    """through the tmfile reader and prerun's shape inference / validation, which run before the device is touched"""
    assert "uint8 graphs only" in _error(S((1, 12, 3, 5), 1, 5, 12, dtype=DT_INT8, in_q=(0.05, 0), out_q=(0.05, 0))[0])
    assert "uint8 graphs only" in _error(S((1, 12, 3, 5), 1, 5, 12, dtype=DT_FP32)[0])
    # the node of shufflenet_v2_benchmark.tmfile's kind: caffe form, two outputs, no slice points
    assert "caffe form" in _error(S((1, 12, 3, 5), 1, 0, 0, iscaffe=1, isonnx=0, outputs=2, out_dims=[1, 6, 3, 5])[0])
    assert "caffe form" in _error(S((1, 12, 3, 5), 1, 0, 0, iscaffe=1, isonnx=0, outputs=2, out_dims=[1, 6, 3, 5], slice_points=[6])[0])
    assert "mxnet form" in _error(S((1, 12, 3, 5), 1, 5, 12, ismxnet=1, isonnx=0)[0])
    assert "tf form" in _error(S((1, 12, 3, 5), 1, 0, 0, isonnx=0, begins=[0, 5, 0, 0], sizes=[1, 7, 3, 5], out_dims=[1, 7, 3, 5])[0])
    assert "one output only" in _error(S((1, 12, 3, 5), 1, 5, 12, outputs=2)[0])
    assert "4-D tensor only" in _error(S((12, 3, 5), 0, 5, 12)[0])
    assert "negative step" in _error(S((1, 12, 3, 5), 1, 5, 12, -1, out_dims=[1, 7, 3, 5])[0])
    assert "negative begin" in _error(S((1, 12, 3, 5), 1, -2, 12, out_dims=[1, 7, 3, 5])[0])
    for begin, end in ((5, 5), (7, 5), (12, 100), (3, -9), (11, -1)):
        assert "begin is not below" in _error(S((1, 12, 3, 5), 1, begin, end, out_dims=[1, 7, 3, 5])[0]), (begin, end)
    for axis in (4, -5, 7):
        assert "outside the tensor's rank" in _error(S((1, 12, 3, 5), axis, 5, 12, out_dims=[1, 7, 3, 5])[0]), axis
    g = tm2.Graph(name="slice_of_const")             # a Slice that reads a constant tensor; the graph's input feeds nothing
    g.add_input("data", [1, 12, 3, 5], DT_UINT8, [lh.f32(0.05)], [77])
    c = g.add_const("table", np.arange(180, dtype=np.uint8).reshape(1, 12, 3, 5), DT_UINT8, [lh.f32(0.05)], [77])
    y = g.add_tensor("out", [1, 7, 3, 5], DT_UINT8, tm2.TT_VAR, None, [lh.f32(0.031)], [12])
    g.output_nodes = [g.add_node("slice", "Slice", [c], [y], axis=1, begin=5, end=12, step=1)]
    assert "must not be a constant" in _error(g)
    g, _ = S((1, 12, 3, 5), 1, 5, 12)
    g.tensors[1].scales, g.tensors[1].zero_points = [lh.f32(0.03)] * 7, [0] * 7
    assert "per-tensor" in _error(g)
    assert "cannot convert to int" in _error(S((1, 12, 3, 5), 1, 5, 12, in_q=(1.0, 0), out_q=(1e-8, 0))[0])
    # .. while the raw copy reads no parameter, and neither does the device
    assert "slice" not in _error(S((1, 12, 3, 5), 1, 0, 12, in_q=(1.0, 0), out_q=(1e-8, 0))[0]).lower()


def test_support_queries():
    L = capi.lib()
    A = so.ask_slice
    assert [L.tamd_op_supported(so.OP_SLICE, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 1]
    # what runs: every case of the GPU tests' single nodes, a stored step of 0, a negative axis
    for case, (axis, begin, end, step) in so.SINGLE.items():
        g, _ = so.gpu_cases()[case]()
        assert A(U8, g.tensors[0].dims, axis, begin, end, step) == 1, case
    assert A(U8, [1, 8, 3, 5], 1, 2, 6, 0) == 1 and A(U8, [1, 3, 7, 5], -2, 2, 6) == 1
    # .. and what does not, each for its own reason
    assert A(I8, [1, 12, 3, 5], 1, 5, 12) == 0 and A(F32, [1, 12, 3, 5], 1, 5, 12) == 0
    assert A(U8, [1, 12, 3, 5], 1, 0, 0, iscaffe=1, isonnx=0, outputs=2, out_dims=[1, 6, 3, 5]) == 0
    assert A(U8, [1, 12, 3, 5], 1, 0, 0, iscaffe=1, isonnx=0, outputs=2, out_dims=[1, 6, 3, 5], slice_point_num=1) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, ismxnet=1, isonnx=0) == 0
    assert A(U8, [1, 12, 3, 5], 1, 0, 0, isonnx=0, begin_num=4, size_num=4, out_dims=[1, 7, 3, 5]) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, outputs=2) == 0
    assert A(U8, [12, 3, 5], 0, 5, 12) == 0 and A(U8, [12, 5], 0, 5, 12) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, const_input=True) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, in_quant=12) == 0 and A(U8, [1, 12, 3, 5], 1, 5, 12, out_quant=7) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, -1, out_dims=[1, 7, 3, 5]) == 0
    assert A(U8, [1, 12, 3, 5], 1, -2, 12, out_dims=[1, 7, 3, 5]) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 5, out_dims=[1, 12, 3, 5]) == 0 and A(U8, [1, 12, 3, 5], 1, 7, 5, out_dims=[1, 7, 3, 5]) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, out_dims=[1, 6, 3, 5]) == 0 and A(U8, [1, 12, 3, 5], 1, 5, 12, out_dims=[1, 7, 3, 4]) == 0
    assert A(U8, [1, 12, 3, 5], 4, 5, 12, out_dims=[1, 7, 3, 5]) == 0
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, in_q=(1.0, 0), out_q=(1e-8, 0)) == 0 and A(U8, [1, 12, 3, 5], 1, 5, 12, out_q=(0.0, 0)) == 0
    assert A(U8, [1, 12, 3, 5], 1, 0, 12, in_q=(1.0, 0), out_q=(1e-8, 0)) == 1          # the raw copy has no byte map
    assert A(U8, [1, 12, 3, 5], 1, 5, 12, with_param=False) == 0
    # the operators that were there keep their answers and their codes; 21 and 24 stay reserved, never-supported values
    assert [L.tamd_op_supported(op, I8) for op in range(26)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1]
    assert [L.tamd_op_supported(op, U8) for op in range(26)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 1]
    assert [L.tamd_op_supported(op, F32) for op in range(26)] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert [L.tamd_op_supported(27, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]


def test_writer_and_reader_round_trip_the_parameter_blob():
    g, _ = S((1, 12, 3, 5), 1, 5, 12)
    node = [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "Slice"]
    assert len(node) == 1 and node[0].params == {"axis": 1, "slice_points": [], "begins": [], "sizes": [], "iscaffe": 0, "ismxnet": 0, "isonnx": 1,
                                                 "begin": 5, "end": 12, "step": 1}
    g, _ = S((1, 12, 3, 5), 1, 0, 0, isonnx=0, begins=[0, 5, 0, 0], sizes=[1, 7, 3, 5], out_dims=[1, 7, 3, 5])
    p = [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "Slice"][0].params
    assert p["begins"] == [0, 5, 0, 0] and p["sizes"] == [1, 7, 3, 5] and p["slice_points"] == [] and p["isonnx"] == 0
    g, _ = S((1, 12, 3, 5), 1, 0, 0, iscaffe=1, isonnx=0, outputs=2, out_dims=[1, 6, 3, 5], slice_points=[6])
    p = [n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "Slice"][0].params
    assert p["slice_points"] == [6] and p["iscaffe"] == 1


@pytest.mark.parametrize("case", ["chan_requant", "batch_axis", "w_step2_odd_width", "chain", "focus", "csp"])
def test_written_tmfile_runs_in_the_reference(ref, case):
    """the reference loads a file tm2.py wrote and runs it; the shape it infers is the one the library infers"""
    g, x = so.gpu_cases()[case]()
    b = tm2.write_tm2(g)
    out = so.reference_outputs(ref, g, x)
    assert len(out) == 1 and out[0].dtype == np.uint8
    shape, err = so.library_outcome(b)
    assert shape == out[0].shape, (shape, out[0].shape, err)
    assert "not supported" not in err and "slice" not in err.lower(), err


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


@pytest.mark.parametrize("case", ["csp", "focus"])
def test_plugin_keeps_the_block_in_one_hip_subgraph(ref, case):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = so.gpu_cases()[case]()
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert len(real) == 1 and real[0][0] == "HIP" and {"Slice", "Concat", "Convolution"} <= set(real[0][1]), real


def test_plugin_leaves_the_refused_forms_and_fp32_to_the_cpu_device(ref):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    c = so.Block(64, DT_FP32, (1, 8, 6, 6))
    c.conv(8, 3, 1); c.slice(1, 4, 8); c.conv(8, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_FP32))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == ["Slice"], real
    c = so.Block(65, DT_UINT8, (1, 8, 6, 6))
    c.conv(8, 3, 1); c.slice(1, 4, 8, ismxnet=1, isonnx=0); c.conv(8, 1)
    g, x = c.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == ["Slice"], real


def test_golden_is_the_real_reference(ref):
    """tests/golden/slice_cases.npz (tools/make_golden_slice.py) holds what the reference computes here, for every GPU case and table"""
    z = so.golden()
    cases = so.gpu_cases()
    stored = {k[:-3] for k in z.files if k.endswith("__n")}
    assert stored == set(cases)
    assert {k[7:] for k in z.files if k.startswith("table__")} == {s[0] for s in so.TABLE_SETS}
    assert os.path.getsize(so.GOLDEN) < 64 * 1024
    for case in sorted(stored):
        g, x = cases[case]()
        want = so.reference_outputs(ref, g, x)
        assert so.equals_golden(z, case, want), case
        want[0].reshape(-1)[0] ^= 1                      # .. and the comparison is one: a single changed bit is seen
        assert not so.equals_golden(z, case, want), case


def test_cases_hold_what_they_are_named_for():
    cases = so.gpu_cases()
    q = lambda g, t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    g, _ = cases["chan_batch2_identity"]()
    assert q(g, 0) == q(g, 1)
    for k in ("full_range_raw_copy", "full_range_end_clipped", "chan_requant"):
        g, _ = cases[k]()
        assert q(g, 0) != q(g, 1), k
    g, _ = cases["chain"]()
    sl = [n for n in g.nodes if n.op == "Slice"]
    assert len(sl) == 2 and sl[1].inputs == sl[0].outputs
    assert len({q(g, sl[0].inputs[0]), q(g, sl[0].outputs[0]), q(g, sl[1].outputs[0])}) == 3
    g, _ = cases["focus"]()
    assert sum(n.op == "Slice" for n in g.nodes) == 8
    g, _ = cases["blocks_ragged"]()
    assert int(np.prod(g.tensors[1].dims)) > 4 * 64 * 16 and int(np.prod(g.tensors[1].dims)) % (64 * 16) != 0
