"""Quantised DepthToSpace on the device (csrc/node_rules.h: depthtospace_refusal; csrc/d2s.hip): device bytes == the real reference
library's bytes, from the committed golden (tests/golden/d2s_cases.npz, always) and from the reference itself (where oracle/_ref is
built), through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, in BOTH forms
(TAMD_PIN=d2s_form=1: d2s_u8 / d2s_i8; 0: the canonical gather of transpose.hip, where the node's output is one dense run -- d2s_helpers.
form0_is_legal -- and the new kernel elsewhere), and through the plugin.  The shapes are the smallest at which the kernels can go wrong:

  uint8 (NCHW), d2s_u8: a lane owns an aligned 16-byte chunk of the image's output run
    u8_rows_of_10               (1,4,3,5) r 2: output rows of 10 bytes, every chunk straddles a row -- the byte walk over rows and planes
    u8_aligned_rows_of_48       (1,8,8,24) r 2: aligned rows of 48 bytes, the two-loads-and-interleave path alone
    u8_r3_batch2                (2,18,2,7) r 3: batch 2, the byte walk with r = 3
    u8_r4_one_pixel             (1,16,1,1) r 4
    u8_r1_copy                  (1,5,3,3) r 1: a copy (slice_u8 in its identity form)
    u8_concat_slice             (1,4,2,8) r 2 written in place into a Concat between neighbours on both sides (planes of 64 bytes: with
                                this shape the slice's offset is a whole number of planes, 192 bytes)
    u8_concat_slice_odd_offset  (1,18,1,1) r 3: two planes of 9 bytes at byte 9 of the Concat's image, neighbours on both sides
  int8 (NHWC), d2s_i8: a lane owns 16 output channels of one output pixel; the inputs hold -128
    i8_outc3_padding            (1,12,3,5) r 2: 3 output channels, 13 padding lanes written as zero; the byte gather
    i8_outc16                   (1,64,4,4) r 2: one full group, the four-loads-and-permute path
    i8_outc20_batch2            (2,80,2,3) r 2: a full group and a quarter-full one, batch 2
    i8_r3                       (1,36,2,2) r 3
    i8_source_concat_slice      the source is channel 16 .. 47 of a Concat's 48-channel pixels, read in place
    i8_into_concat_in_place     the output is written into the buffer of a Concat of two inputs: -128 comes out as the reference's Concat
                                stores it (127); i8_into_concat_copied: 3 channels, the Concat copies and does the same
  {i8,u8}_espcn_tail, {i8,u8}_edsr_upsampler   the two sub-pixel-convolution graphs at (1,8,6,6), r 2, also through the plugin"""
import ctypes as C
import os

import numpy as np
import pytest

import d2s_helpers as dh
import lut_helpers as lh
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dh.gpu_cases()
OURS = ("d2s_u8", "d2s_i8", "transpose_gather_q8", "slice_u8")


@pytest.fixture(scope="module")
def golden():
    return dh.golden()


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


def _run_case(case, golden):
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes.  Returns the kernels of
    the DepthToSpace nodes' launches in the pooled run, and the outputs"""
    dtype, build = CASES[case]
    g, x = build()
    b = tm2.write_tm2(g)
    names = {n.name for n in g.nodes if n.op == "DepthToSpace"}
    want = dh.reference_outputs(ref_capi, g, x, dtype) if ref_capi.available() else None
    profs = []
    for keep in (False, True):
        got, prof = _device(b, x, keep_tensors=keep)
        profs.append([(k["node"], k["kernel"]) for k in prof])
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert dh.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    assert profs[0] == profs[1]
    return [k for node, k in profs[0] if node in names and k in OURS], got


def _pinned(key, value, fn):
    old = os.environ.get("TAMD_PIN")
    os.environ["TAMD_PIN"] = "%s=%d" % (key, value)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["TAMD_PIN"]
        else:
            os.environ["TAMD_PIN"] = old


@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("case", sorted(CASES))
def test_both_forms_give_the_references_bytes_in_one_launch(case, form, golden):
    kernels, got = _pinned("d2s_form", form, lambda: _run_case(case, golden))
    assert kernels == dh.expected_kernels(case, form), (case, form, kernels)
    if case in dh.SINGLE:
        dt, dims, r = dh.SINGLE[case]
        assert np.array_equal(got[0], dh.numpy_d2s(CASES[case][1]()[1], r))


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("dims", [(1, 64, 128, 128), (1, 64, 128, 127)], ids=["1MiB", "just_below"])
def test_the_default_form_follows_the_measured_threshold(dims, dtype):
    """profiles/d2s.txt: with nothing pinned the new kernel runs from 1 MiB of output on and the gather below -- the two shapes sit on
    both sides of the threshold, 16 output channels (form 0 is legal in int8 too); the bytes are the numpy statement's either way"""
    g, x = dh.d2s_graph(dtype, dims, 2)
    want = dh.numpy_d2s(x, 2)
    assert (want.size >= dh.NEW_FORM_FROM_BYTES) == (dims[3] == 128) and abs(want.size - dh.NEW_FORM_FROM_BYTES) < 16384
    got, prof = _device(tm2.write_tm2(g), x)
    assert np.array_equal(got[0], want)
    kernels = [k["kernel"] for k in prof if k["kernel"] in OURS]
    new = "d2s_i8" if dtype == DT_INT8 else "d2s_u8"
    assert kernels == ([new] if dh.default_form(dims) else ["transpose_gather_q8"]), kernels


def test_small_cases_default_to_the_gather_where_it_is_legal(golden):
    for case in ("u8_aligned_rows_of_48", "i8_outc16", "i8_outc3_padding", "u8_concat_slice"):
        kernels, _ = _run_case(case, golden)
        assert kernels == dh.expected_kernels(case, 0), (case, kernels)


def test_every_case_is_run():
    assert set(dh.SINGLE) < set(CASES) and len(CASES) == len(dh.SINGLE) + 9
    assert sum(dh.form0_is_legal(c) for c in CASES) >= 10 and not all(dh.form0_is_legal(c) for c in CASES)


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("build", [dh.espcn_tail, dh.edsr_upsampler], ids=["espcn_tail", "edsr_upsampler"])
def test_plugin_runs_sub_pixel_convolution_as_one_hip_subgraph(ref, build, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  One "HIP" subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the
    copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator
    table cannot know this operator (tests/test_gpu_shuffle.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = build(dtype)
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
        assert dh.REF_OP_NAME in real[0][1], pl
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
