"""Quantised nearest Resize on the device (csrc/node_rules.h: resize_refusal; csrc/interp.hip fed with Resize's operands, csrc/resize.hip):
device bytes == the real reference library's bytes, from the committed golden (tests/golden/resize_cases.npz, always) and from the
reference itself (where oracle/_ref is built), through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per
graph, in BOTH forms -- TAMD_PIN=resize_form=0: interp_nearest_i8 / interp_nearest_u8; 1: resize_rep_i8 / resize_rep_u8 where the index
vectors are those of whole-number factors (resize_helpers.rep_is_legal), form 0 elsewhere -- with the kernel's name taken from the launch
list and the two forms' bytes compared with each other, and through the plugin.  All batch 1; every byte is compared.  The shapes are the
smallest at which the kernels can go wrong:

  int8 (NHWC): a lane owns 16 channels of one pixel (form 0: an output pixel; form 1: a source pixel, stored sh * sw times)
    i8_c1 / c16 / c17 / c40     (1,C,3,5) x2: one channel and 15 padding lanes written as zero, one full vector, a full one and one
                                channel, two full ones and a half
    i8_scale_*                  (1,24,6,10) at (2,2), (2,3), (3,1), (1,1), (1.5,2.5), (0.5,0.5): the last two are form 0 under either pin
    i8_equal_minus128           equal parameters and -128 in the input: it comes out as -127
    i8_source_concat_view       the source is channel 16 .. 47 of a Concat's 48-channel pixels (cs_in 48 > C 32), read in place
    i8_into_concat_resize_first / _last   the output is channels 16 .. 31 of a Concat's 48, written in place, the neighbours on both
                                sides written by convolutions planned behind / in front of the node
  uint8 (NCHW): a lane owns an aligned 16-byte chunk of the output run
    u8_planes_of_60             (1,3,3,5) x2: planes of 6 x 10 = 60 bytes, never aligned, OW 10 < 16: the byte walk over rows and planes
    u8_rows_of_18               W 9 -> OW 18: chunks across a row boundary, and whole chunks inside a row (the doubling path)
    u8_rows_of_48               aligned rows: the doubling path alone;  u8_rows_of_36_h3: sw 2 under sh 3, chunks starting at columns
                                0, 16, 32 -> 12, ... (with sw 2 every row and plane is even, so a whole chunk never starts at an odd
                                column in an aligned buffer: resize.hip says why the nine-byte form is not built)
    u8_sw3, u8_scale_1_1        the byte walk at sw 3 and the copy;  u8_shrink, u8_non_integer: form 0 under either pin
    u8_identity_x2 / _sw3       equal parameters: no lookups, on the doubling path and on the byte walk
    u8_into_concat_odd_offset_resize_first / _last   x3: two planes of 81 bytes at byte 81 of a Concat's image, neighbours on both sides
    u8_into_concat_x2           x2: planes of 144 bytes behind one of a neighbour
  {i8,u8}_neck_block            conv -> Resize x2 -> Concat(skip) -> conv3x3 whole, also through the plugin"""
import ctypes as C
import os

import numpy as np
import pytest

import lut_helpers as lh
import resize_helpers as rh
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rh.gpu_cases()
OURS = ("resize_rep_i8", "resize_rep_u8", "interp_nearest_i8", "interp_nearest_u8")


@pytest.fixture(scope="module")
def golden():
    return rh.golden()


@pytest.fixture(scope="module")
def reference():
    """the reference's outputs of every case, computed once (where oracle/_ref is built)"""
    if not ref_capi.available():
        return {}
    out = {}
    for case, (dtype, build) in CASES.items():
        g, x = build()
        out[case] = rh.reference_outputs(ref_capi, g, x, dtype)
    return out


def _device(b, x, **kw):
    gr = capi.Graph(b, **kw)
    gr.set_input(x)
    out = gr.run()
    prof = gr.profile(1)
    again = gr.run()                                     # (after the profiling pass: the launches are idempotent)
    gr.close()
    for a, c in zip(out, again):
        assert np.array_equal(a, c)
    return out, prof


def _run_case(case, golden, want):
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes.  Returns the kernels of
    the Resize nodes' launches in the pooled run, and the outputs"""
    dtype, build = CASES[case]
    g, x = build()
    b = tm2.write_tm2(g)
    names = {n.name for n in g.nodes if n.op == "Resize"}
    profs = []
    for keep in (False, True):
        got, prof = _device(b, x, keep_tensors=keep)
        profs.append([(k["node"], k["kernel"]) for k in prof])
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert rh.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    assert profs[0] == profs[1]
    if "into_concat" in case:                            # written IN PLACE, the neighbours too: the Concat launches nothing
        assert not [k for _, k in profs[0] if k.startswith("concat")], profs[0]
    return [k for node, k in profs[0] if node in names], got


def _pinned(form, fn):
    old = os.environ.get("TAMD_PIN")
    os.environ["TAMD_PIN"] = "resize_form=%d" % form
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["TAMD_PIN"]
        else:
            os.environ["TAMD_PIN"] = old


@pytest.mark.parametrize("case", sorted(CASES))
def test_both_forms_give_the_references_bytes_in_one_launch(case, golden, reference):
    want = reference.get(case)
    outs = {}
    for form in (0, 1):
        kernels, outs[form] = _pinned(form, lambda: _run_case(case, golden, want))
        assert kernels == [rh.expected_kernel(case, form)], (case, form, kernels)
    for a, b in zip(outs[0], outs[1]):
        assert a.dtype == b.dtype and np.array_equal(a, b), case     # the two forms, byte for byte
    if case in rh.SINGLE:
        dt, dims, p, kw = rh.SINGLE[case]
        iq, oq = kw.get("in_q", rh.IN_Q[dt]), kw.get("out_q", rh.OUT_Q[dt])
        x = CASES[case][1]()[1]
        assert np.array_equal(outs[1][0], rh.numpy_resize(x, p, capi.resize_table(dt, lh.f32(iq[0]), iq[1], lh.f32(oq[0]), oq[1])))


def _unpinned(fn):
    old = os.environ.pop("TAMD_PIN", None)
    try:
        return fn()
    finally:
        if old is not None:
            os.environ["TAMD_PIN"] = old


@pytest.mark.parametrize("dtype,dims", [(DT_UINT8, (1, 256, 40, 40)), (DT_UINT8, (1, 255, 40, 40)), (DT_INT8, (1, 256, 80, 80)), (DT_INT8, (1, 240, 80, 80))],
                         ids=["uint8_1638400", "uint8_just_below", "int8_6553600", "int8_just_below"])
def test_the_default_form_follows_the_measured_threshold(dtype, dims):
    """profiles/resize.txt: with nothing pinned the replicate kernel runs from 1 638 400 (uint8) / 6 553 600 (int8) output bytes on and
    interp.hip's kernel below -- the shapes sit on both sides of each threshold; the bytes are the numpy statement's either way"""
    p = rh.scales(2.0)
    g, x = rh.single(dtype, dims, p, 5)
    iq, oq = rh.IN_Q[dtype], rh.OUT_Q[dtype]
    want = rh.numpy_resize(x, p, capi.resize_table(dtype, lh.f32(iq[0]), iq[1], lh.f32(oq[0]), oq[1]))
    assert (want.size >= rh.REP_FROM_BYTES[dtype]) == (dims[1] == 256) and abs(want.size - rh.REP_FROM_BYTES[dtype]) <= 16 * 160 * 160
    got, prof = _unpinned(lambda: _device(tm2.write_tm2(g), x))
    assert np.array_equal(got[0], want)
    kernels = [k["kernel"] for k in prof if k["kernel"] in OURS]
    t = "i8" if dtype == DT_INT8 else "u8"
    assert kernels == [("resize_rep_" if rh.default_form(dtype, want.shape) else "interp_nearest_") + t], kernels


def test_small_cases_default_to_form_0(golden, reference):
    for case in ("i8_scale_2_2", "u8_rows_of_48", "i8_into_concat_resize_last", "u8_neck_block"):
        kernels, _ = _unpinned(lambda: _run_case(case, golden, reference.get(case)))
        assert kernels == [rh.expected_kernel(case, 0)], (case, kernels)


def test_every_case_is_run():
    assert set(rh.SINGLE) < set(CASES) and len(CASES) == len(rh.SINGLE) + 8
    assert sum(rh.rep_is_legal(c) for c in CASES) >= 20 and sum(not rh.rep_is_legal(c) for c in CASES) == 4


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_runs_the_neck_block_as_one_hip_subgraph(ref, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  One "HIP" subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the
    copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator
    table cannot know this operator (tests/test_gpu_shuffle.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = rh.neck_block(dtype)
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
        assert rh.REF_OP_NAME in real[0][1], pl
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
