"""Quantised Transpose on the device (csrc/transpose_tables.cc + transpose.hip): device bytes == the real reference library's bytes, from
the committed golden (tests/golden/transpose_cases.npz, always) and from the reference itself (where oracle/_ref is built), through the
C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, and through the plugin.  The shapes are the smallest
at which each path of the three kernels can go wrong:

  u8_2d .. u8_6d          one Transpose between graph input and output, ranks 2 .. 6: every order the issue names, in every legal form
  u8_4d_identity_order    order (0, 1, 2, 3) between different parameters: the pure byte map, not a copy
  u8_size1_axes           (1, 1, 5, 1, 7) reversed: the size-1 axes drop out of the geometry
  u8_tile_edges_65x67     (1, 65, 67) order (0, 2, 1): ragged tiles on both axes, four tiles, planes at odd byte offsets
  u8_tile_edges_130x3     (3, 130, 3): three tiles along one axis, three bytes along the other, a batch axis in the grid
  u8_rows_L               (2, 3, L) order (1, 0, 2), L = 1, 15, 16, 17, 33: chunks that cross runs, unaligned sources
  u8_equal_params_*       the form without table;  u8_coarser: a pair that does not saturate (every other uint8 case saturates at 0 and 255)
  i8_input_nhwc_minus128  int8 graph input (2, 6, 4, 5), order (0, 2, 3, 1), read where it lies in 16-byte pixels; -128 comes out as -127
  i8_input_saturates      .. between scales 0.05 and 0.02: +-127
  i8_view                 conv (6 channels, 16-byte pixels) -> Reshape (1, 2, 3, 20) -> Transpose: one launch, or two with transpose_view=0
  i8_concat_view          the same behind a Concat (20 channels, 32-byte pixels), and a Transpose that reads a channel slice at offset 16
  i8_mixed_reshape        a Reshape that mixes C and H: two launches by rule
  i8_dense_chain          Reshape -> Transpose -> Transpose: the second reads a dense tensor
  i8_detect, u8_detect    the Detect head at two scales, batch 2;  u8_shuffle: torch's channel shuffle;  u8_batch_axis: order[0] != 0"""
import ctypes as C
import os

import numpy as np
import pytest

import lut_helpers as lh
import transpose_helpers as th
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = th.gpu_cases()
RAN = set()
GATHER, ROWS, TILE = "transpose_gather_q8", "transpose_rows_q8", "transpose_tile_q8"
FORM = {0: GATHER, 1: ROWS, 2: TILE}
# which of rows / tile the canonical geometry of each single-node case is legal in: rows where the output's innermost axis is the input's
# stride-1 axis (or what is left of it after merging), tile otherwise.  (2, 3, 1) order (1, 0, 2): the run of ONE byte is a size-1 axis
# and drops out -- what is left is a 2-D transpose, the tile form
LEGAL = {k: TILE for k in th.U8_SINGLE}
LEGAL.update({k: ROWS for k in ("u8_3d_102", "u8_4d_identity_order", "u8_5d_shuffle", "u8_rows_15", "u8_rows_16", "u8_rows_17", "u8_rows_33", "u8_equal_params_rows")})


@pytest.fixture(scope="module")
def golden():
    return th.golden()


def _device(b, x, **kw):
    gr = capi.Graph(b, **kw)
    gr.set_input(x)
    out = gr.run()
    prof = gr.profile(1)
    again = gr.run()                                     # (after the profiling pass: the launches are idempotent)
    halves = gr.halves()
    gr.close()
    for a, c in zip(out, again):
        assert np.array_equal(a, c)
    return out, prof, halves


def _run_case(case, golden, **kw):
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes.  Returns the launch
    list of the pooled run and the outputs"""
    RAN.add(case)
    dtype, build = CASES[case]
    g, x = build()
    b = tm2.write_tm2(g)
    want = th.reference_outputs(ref_capi, g, x, dtype) if ref_capi.available() else None
    profs = []
    for keep in (False, True):
        got, prof, halves = _device(b, x, keep_tensors=keep, **kw)
        assert halves == 0
        profs.append([(k["node"], k["kernel"]) for k in prof])
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (case, keep, int((w != o).sum()), w.size)
        assert th.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    assert profs[0] == profs[1]
    return profs[0], got


def _pinned(pins, fn):
    old = os.environ.get("TAMD_PIN")
    os.environ["TAMD_PIN"] = ",".join("%s=%d" % kv for kv in pins.items())
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["TAMD_PIN"]
        else:
            os.environ["TAMD_PIN"] = old


def _kernels(prof, names=(GATHER, ROWS, TILE)):
    return [(n, k) for n, k in prof if k in names]


@pytest.mark.parametrize("case", sorted(th.U8_SINGLE))
def test_uint8_transpose_bytes_are_the_references_in_every_legal_form(case, golden):
    """one launch under the node's name; transpose_form = 0 | 1 | 2 pins the gather, the rows form, the tile form where the geometry is
    legal for it (the default form where it is not): the same bytes, which are also capi.transpose_table(..)[np.transpose(x, order)]"""
    dims, order, in_q, out_q = th.U8_SINGLE[case]
    g, x = CASES[case][1]()
    want = th.table_of(DT_UINT8, in_q or th.U8_IN, out_q or th.U8_OUT)[np.transpose(x, order)]
    default, got = _run_case(case, golden)
    assert default == [("transpose", GATHER)], default  # (below 8 MiB: test_default_form_at_the_tile_threshold)
    assert np.array_equal(got[0], want)
    seen = set()
    for form in (0, 1, 2):
        prof, out = _pinned({"transpose_form": form}, lambda: _run_case(case, golden))
        assert len(prof) == 1 and prof[0][0] == "transpose", prof
        assert prof[0][1] in (FORM[form], GATHER), (form, prof)                   # the pinned form, or the default where it is not legal
        seen.add(prof[0][1])
        assert np.array_equal(out[0], want), (case, form)
    assert seen == {GATHER, LEGAL[case]}, seen           # rows and tile exclude each other, and one of them is legal for every case here


def test_default_form_at_the_tile_threshold():
    """the tile form is the default from 8 MiB on (transpose_default_form: where it was measured ahead of the gather), the gather below:
    (2, 2048, 2048) and (2, 2047, 2048) order (0, 2, 1), equal parameters -- the bytes are np.transpose of the input either way"""
    for rows, kernel in ((2048, TILE), (2047, GATHER)):
        g, x = th.transpose_graph(DT_UINT8, (2, rows, 2048), (0, 2, 1), (0.05, 77), (0.05, 77), seed=9)
        got, prof, _ = _device(tm2.write_tm2(g), x)
        assert [(k["node"], k["kernel"]) for k in prof] == [("transpose", kernel)], (rows, prof)
        assert np.array_equal(got[0], np.transpose(x, (0, 2, 1)))


@pytest.mark.parametrize("case", ["i8_input_nhwc_minus128", "i8_input_saturates"])
def test_int8_graph_input_is_read_where_it_lies(case, golden):
    """(2, 6, 4, 5) order (0, 2, 3, 1): six channels in 16-byte pixels -- runs of 6 bytes, legal for the rows form; every form the same"""
    g, x = CASES[case][1]()
    q = lambda t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    want = th.table_of(DT_INT8, q(0), q(1))[np.transpose(x, (0, 2, 3, 1)).view(np.uint8)]
    for form in (-1, 0, 1, 2):
        prof, got = _run_case(case, golden) if form < 0 else _pinned({"transpose_form": form}, lambda: _run_case(case, golden))
        assert prof == [("transpose", ROWS if form == 1 else GATHER)], (form, prof)
        assert np.array_equal(got[0], want)
    if case == "i8_input_nhwc_minus128":
        assert (x == -128).sum() >= 7 and (got[0] == -128).sum() == 0 and (got[0] == -127).sum() >= (x == -128).sum()
    else:
        assert (got[0] == 127).sum() > 1 and (got[0] == -127).sum() > 1


def test_int8_reshape_transpose_of_a_convolution_is_one_launch(golden):
    """the view form: no reshape_i8; TAMD_PIN=transpose_view=0: two launches, the same bytes"""
    one, a = _run_case("i8_view", golden)
    two, b = _pinned({"transpose_view": 0}, lambda: _run_case("i8_view", golden))
    assert _pinned({"transpose_view": 1}, lambda: _run_case("i8_view", golden))[0] == one
    assert [k for _, k in one if k == "reshape_i8"] == [] and _kernels(one) == [("reshape2+transpose3", GATHER)], one
    assert [(n, k) for n, k in two if k == "reshape_i8" or k in FORM.values()] == [("reshape2", "reshape_i8"), ("transpose3", GATHER)], two
    assert np.array_equal(a[0], b[0])
    # through the Reshape the output's innermost axis is the pixel axis (16 bytes apart), the stride-1 axis the 3 channels of a group: tile
    # is legal; the dense copy has the 20 pixels innermost on both sides: rows is
    for pins, kernels in (({"transpose_form": 2}, [("reshape2+transpose3", TILE)]), ({"transpose_form": 1}, [("reshape2+transpose3", GATHER)]),
                          ({"transpose_form": 1, "transpose_view": 0}, [("transpose3", ROWS)]), ({"transpose_form": 2, "transpose_view": 0}, [("transpose3", GATHER)])):
        prof, c = _pinned(pins, lambda: _run_case("i8_view", golden))
        assert _kernels(prof) == kernels and np.array_equal(a[0], c[0]), (pins, prof)


def test_int8_view_behind_a_concat_and_a_channel_slice(golden):
    """Reshape -> Transpose of a Concat's 20 channels in 32-byte pixels: one launch; the Transpose of a 16-channel convolution that is
    written in place at channel 16 of another Concat's buffer reads it there"""
    one, a = _run_case("i8_concat_view", golden)
    assert [k for _, k in one if k == "reshape_i8"] == [], one
    assert [n for n, _ in _kernels(one)] == ["reshape4+transpose5", "transpose10"], one
    two, b = _pinned({"transpose_view": 0}, lambda: _run_case("i8_concat_view", golden))
    assert [n for n, k in two if k == "reshape_i8"] == ["reshape4"], two
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert [k for _, k in _kernels(one)] == [GATHER, GATHER]
    t, c = _pinned({"transpose_form": 2}, lambda: _run_case("i8_concat_view", golden))
    r, d = _pinned({"transpose_form": 1}, lambda: _run_case("i8_concat_view", golden))
    assert [k for _, k in _kernels(t)] == [TILE, GATHER] and [k for _, k in _kernels(r)] == [GATHER, ROWS]      # (20 pixels 32 bytes apart; 16 channels side by side)
    for x, y, z in zip(a, c, d):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_int8_reshape_that_mixes_channels_and_rows_keeps_its_copy(golden):
    prof, _ = _run_case("i8_mixed_reshape", golden)
    assert [(n, k) for n, k in prof if k == "reshape_i8" or k in FORM.values()] == [("reshape2", "reshape_i8"), ("transpose3", GATHER)], prof


def test_int8_transpose_of_a_dense_tensor(golden):
    prof, _ = _run_case("i8_dense_chain", golden)
    assert _kernels(prof) == [("reshape2+transpose3", GATHER), ("transpose4", GATHER)], prof
    prof, _ = _pinned({"transpose_form": 2}, lambda: _run_case("i8_dense_chain", golden))
    assert _kernels(prof) == [("reshape2+transpose3", TILE), ("transpose4", TILE)], prof


@pytest.mark.parametrize("case", ["i8_detect", "u8_detect"])
def test_detect_head(case, golden):
    """two scales: per scale conv -> (Reshape) -> Transpose -> Sigmoid -> (Reshape); one Concat.  int8 reads the convolution's NHWC buffer
    through the Reshape (runs of 7 bytes: the rows form is the legal one), uint8 moves (7, H * W) per anchor (the tile form is)"""
    prof, got = _run_case(case, golden)
    assert [k for _, k in prof if k == "reshape_i8"] == [], prof
    assert [k for _, k in _kernels(prof)] == [GATHER] * 2, prof
    for form in (1, 2):
        p2, g2 = _pinned({"transpose_form": form}, lambda: _run_case(case, golden))
        assert [k for _, k in _kernels(p2)] == [FORM[form] if (form == 1) == (case[0] == "i") else GATHER] * 2, (form, p2)
        assert np.array_equal(got[0], g2[0])
    assert [k for _, k in prof].count("lut_u8") == 2, prof
    if case == "i8_detect":
        assert len(prof) == 8, prof                      # conv, transpose, lut; pool, conv, transpose, lut; concat
        two, _ = _pinned({"transpose_view": 0}, lambda: _run_case(case, golden))
        assert [k for _, k in two].count("reshape_i8") == 2 and len(two) == 10, two


def test_onnx_channel_shuffle_uint8(golden):
    prof, _ = _run_case("u8_shuffle", golden)
    assert _kernels(prof) == [("transpose3", GATHER)], prof
    assert [n for n, _ in prof if not n.startswith("conv")] == ["transpose3"], prof      # the Reshapes are views
    prof, _ = _pinned({"transpose_form": 1}, lambda: _run_case("u8_shuffle", golden))
    assert _kernels(prof) == [("transpose3", ROWS)], prof


def test_transpose_of_the_batch_axis_is_not_split_by_batch(golden):
    """every tensor carries 4 as dimension 0: with split_batch = 2 the graph would be two half-batch graphs but for the Transpose"""
    prof, got = _run_case("u8_batch_axis", golden, direct_dispatch=True, split_batch=2)
    assert _kernels(prof) == [("transpose2", GATHER)], prof


def test_every_case_is_run():
    assert RAN == set(CASES), set(CASES) ^ RAN


@pytest.mark.parametrize("case", ["i8_detect", "u8_detect", "u8_shuffle"])
def test_plugin_runs_the_block_as_one_hip_subgraph(ref, case):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  One "HIP" subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the
    copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator
    table cannot know this operator (tests/test_gpu_shuffle.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    dtype, build = CASES[case]
    g, x = build()
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, dtype)
    want = ref.run_model(b, x, mode)
    rg = ref.RefGraph(b, mode, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = tp.placement(rg)
    got = rg.outputs()
    rg.run()
    again = rg.outputs()
    rg.close()
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert any(dev == "HIP" for dev, _ in real), pl
    if built_here:
        assert len(real) == 1 and real[0][0] == "HIP", (tp.PLUGIN, pl)
        assert "Transpose" in real[0][1], pl
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
