"""uint8 Crop on the device (csrc/node_rules.h: crop_refusal; slice.hip, interp.hip, topdown.hip): device bytes == the real reference
library's bytes, from the committed golden (tests/golden/crop_cases.npz, always) and from the reference itself (where oracle/_ref is
built), through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, and through the plugin.  The
shapes are the smallest at which each path can go wrong:

  a Crop alone -- one slice_u8 launch in its identity form; input and output tensors carry different parameters in every case
    retina_cut              (1,8,16,20) -> (1,8,15,20): RetinaFace's own cut, whole rows
    offsets_hw              .. -> (1,8,14,17) from (1, 2): rows of 17 bytes out of rows of 20
    caffe_axis1_c3          (1,8,6,7) -> (1,5,5,6), axis 1, offset_c 3: the channel offset
    axis2_ignores_offset_c  .. the same node with axis 2: offset_c is not read
    mxnet_args2             (1,4,9,11) -> (1,4,7,8), flag 1, num_args 2
    whole_input             (1,3,5,7) -> itself: a plain copy
    no_aligned_row          (1,3,5,7) -> (1,3,4,5): no row and no plane starts aligned
    batch2                  (2,4,8,10) -> (2,4,7,9): the image stride
    ragged_blocks           (2,5,37,41) -> (2,5,33,40): several blocks per image, the last one partial
  Interp -> Crop -- one interp_nearest_u8 launch with shifted index vectors; TAMD_PIN=crop_chain=0: two launches
    chain_x2_identity_map   x2 of (1,8,8,10) cut to (15,20), equal parameters on both sides of the Interp
    chain_x2_off11          .. cut to (15,19) from (1,1), a byte map that is not the identity
    chain_scale15           scale 1.5: (12,15) cut to (11,13) from (1,2)
    chain_batch2            (2,3,8,10)
    chain_second_reader     two Crops read the Interp: nothing is fused
  Interp -> Crop -> Eltwise -- with TAMD_PIN=topdown=1 one topdown_u8 launch; TAMD_PIN=topdown=0 (the default): the chain and eltwise_u8
    td_{prod,sum,sub,max}_{first,second}   every type, the cropped operand listed first and second, two parameter sets
    td_w19_c3_offset        (1,3,15,19) from (1,1): W = 19, H * W = 285 -- chunks straddle rows and planes; a third parameter set
    td_batch2_ragged        (2,5,15,19): three blocks, the last one partial, a ragged last chunk
    td_saturating           results below 0 and above 255
    td_narrow_batch2_offset (2,3,7,9) from (1,1): a map narrower than 16 -- every chunk walks byte by byte over several rows, and row and
                            plane wraps inside the walk feed the gathers behind them
    td_tiny_planes          (1,3,3,5) from (1,1): planes of 15 bytes, two plane crossings inside one chunk
    td_wide_rows            (1,1,2,520): OW > 512, the column indices are read from memory instead of LDS
    nf_cut_channels, nf_gate, nf_second_reader   a box that cuts channels, a gate-form Eltwise, a second reader: not fused
  pyramid                   RetinaFace's merge between convolutions, also through the plugin"""
import ctypes as C
import os

import numpy as np
import pytest

import crop_helpers as ch
import lut_helpers as lh
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ch.gpu_cases()
OURS = ("interp_nearest_u8", "slice_u8", "eltwise_u8", "topdown_u8", "chan_gate_u8")


@pytest.fixture(scope="module")
def golden():
    return ch.golden()


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
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes.  Returns the kernels
    of the pooled run that this operator is about, in launch order, and the outputs"""
    g, x = CASES[case]()
    b = tm2.write_tm2(g)
    want = ch.reference_outputs(ref_capi, g, x) if ref_capi.available() else None
    profs = []
    for keep in (False, True):
        got, prof = _device(b, x, keep_tensors=keep)
        profs.append([(k["node"], k["kernel"]) for k in prof])
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert ch.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    assert profs[0] == profs[1]
    return [k for _, k in profs[0] if k in OURS], got


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


@pytest.mark.parametrize("case", sorted(ch.SINGLE))
def test_crop_alone_is_one_slice_launch_of_the_inputs_own_bytes(case, golden):
    kernels, got = _run_case(case, golden)
    assert kernels == ["slice_u8"], kernels
    x_dims, like, p = ch.SINGLE[case]
    _, x = CASES[case]()
    assert np.array_equal(got[0], ch.numpy_crop(x, like, p))


@pytest.mark.parametrize("case", ["chain_x2_identity_map", "chain_x2_off11", "chain_scale15", "chain_batch2"])
def test_interp_crop_chain_fused_and_as_two_launches(case, golden):
    """the default shifts the Interp's index vectors: ONE interp_nearest_u8 launch, no slice_u8; TAMD_PIN=crop_chain=0 runs both"""
    fused, a = _run_case(case, golden)
    two, b = _pinned("crop_chain", 0, lambda: _run_case(case, golden))
    assert _pinned("crop_chain", 1, lambda: _run_case(case, golden))[0] == fused
    assert fused == ["interp_nearest_u8"], fused
    assert two == ["interp_nearest_u8", "slice_u8"], two
    assert np.array_equal(a[0], b[0])


def test_interp_with_a_second_reader_is_not_fused(golden):
    kernels, got = _run_case("chain_second_reader", golden)
    assert kernels == ["interp_nearest_u8", "slice_u8", "slice_u8"], kernels
    assert len(got) == 2


@pytest.mark.parametrize("case", sorted(ch.TOPDOWN))
def test_topdown_merge_is_one_launch(case, golden):
    """TAMD_PIN=topdown=1: ONE topdown_u8 launch and none of the three kernels it replaces; TAMD_PIN=topdown=0: the chain form and
    eltwise_u8; the reference's bytes both ways"""
    fused, a = _pinned("topdown", 1, lambda: _run_case(case, golden))
    chain, b = _pinned("topdown", 0, lambda: _run_case(case, golden))
    assert fused == ["topdown_u8"], fused
    assert chain == ["interp_nearest_u8", "eltwise_u8"], chain
    assert np.array_equal(a[0], b[0])


def test_topdown_needs_the_chain_form(golden):
    """TAMD_PIN=crop_chain=0 alone gives three launches: the merge builds on the chain"""
    three, _ = _pinned("crop_chain", 0, lambda: _run_case("td_sub_first", golden))
    assert three == ["interp_nearest_u8", "slice_u8", "eltwise_u8"], three


@pytest.mark.parametrize("case,want", [("nf_cut_channels", ["interp_nearest_u8", "slice_u8", "eltwise_u8"]), ("nf_gate", ["interp_nearest_u8", "chan_gate_u8"]),
                                       ("nf_second_reader", ["interp_nearest_u8", "eltwise_u8"])])
def test_what_is_not_a_topdown_merge_is_not_fused(case, want, golden):
    """a box that cuts channels keeps its three launches; a gate-form Eltwise and a Crop output with a second reader keep the chain"""
    kernels, _ = _pinned("topdown", 1, lambda: _run_case(case, golden))
    assert kernels == want, kernels


def test_pyramid_block(golden):
    fused, a = _pinned("topdown", 1, lambda: _run_case("pyramid", golden))
    plain, b = _pinned("topdown", 0, lambda: _run_case("pyramid", golden))
    assert fused == ["topdown_u8"] and plain == ["interp_nearest_u8", "eltwise_u8"], (fused, plain)
    assert np.array_equal(a[0], b[0])
    # the default is what was measured ahead (profiles/crop_topdown.txt): the chain form and eltwise_u8; topdown_u8 is opt-in
    assert _run_case("pyramid", golden)[0] == plain


def test_every_case_is_run():
    assert set(ch.SINGLE) | set(ch.CHAINS) | set(ch.TOPDOWN) | set(ch.NOT_FUSED) | {"pyramid"} == set(CASES)


def test_plugin_runs_the_pyramid_block_as_one_hip_subgraph(ref):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  One "HIP" subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the
    copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator
    table cannot know this operator (tests/test_gpu_shuffle.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = ch.pyramid_graph(DT_UINT8)
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, DT_UINT8)
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
        assert "Crop" in real[0][1], pl
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
