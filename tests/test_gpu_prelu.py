"""Quantised PReLU on the device (csrc/prelu_tables.cc + prelu.hip: prelu_i8, prelu_u8): device bytes == the real reference library's
bytes, from the committed golden (tests/golden/prelu_cases.npz, always) and from the reference itself (where oracle/_ref is built),
through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, and through the plugin.  The all-bytes
graphs are also held against tamd_prelu_table directly: every byte of every channel.  The shapes are the smallest at which the kernels
can go wrong: int8 with 11 padding lanes, none, and a second quarter-full 16-lane group; uint8 planes of 49 bytes (unaligned starts, a
head and a tail in every plane), of one byte, of 335 bytes (whole chunks between two ragged ones), and aligned ones."""
import ctypes as C
import os

import numpy as np
import pytest

import lut_helpers as lh
import prelu_helpers as ph
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ph.gpu_cases()
KERNEL = {DT_INT8: "prelu_i8", DT_UINT8: "prelu_u8"}


@pytest.fixture(scope="module")
def golden():
    return ph.golden()


def _device(b, x, **kw):
    gr = capi.Graph(b, **kw)
    gr.set_input(x)
    out = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    again = gr.run()                                     # (after the profiling pass: the launches are idempotent)
    gr.close()
    for a, c in zip(out, again):
        assert np.array_equal(a, c)
    return out, names


def _run_case(case, golden, prelus):
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes; the launch list names
    prelu_i8 / prelu_u8 once per node.  Returns the outputs of the pooled run"""
    dtype, build = CASES[case]
    g, x = build()
    assert np.array_equal(golden[case + "__in"], x)
    b = tm2.write_tm2(g)
    want = ph.reference_outputs(ref_capi, g, x, dtype) if ref_capi.available() else None
    first = None
    for keep in (False, True):
        got, names = _device(b, x, keep_tensors=keep)
        assert names.count(KERNEL[dtype]) == prelus and names.count(KERNEL[DT_UINT8 if dtype == DT_INT8 else DT_INT8]) == 0, names
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert ph.equals_golden(golden, case, got), (case, keep, [int((golden["%s__out%d" % (case, i)] != o).sum()) for i, o in enumerate(got)])
        first = first or got
    return first


@pytest.mark.parametrize("case", ph.ALL_BYTES_SETS, ids=[s[0] for s in ph.ALL_BYTES_SETS])
def test_every_byte_of_every_channel(case, golden):
    """(1, C, 16, 16), every channel all 256 byte values, a slope per channel that reaches every branch (0.25 and 4.0, which act as 0;
    0; 0.1; a negative one; 3.3 into saturation; a sub-normal half; -0): the device equals the reference AND tamd_prelu_table.  This is
    where a wrong per-channel index or a wrong near-tie of the int8 requantisation shows"""
    got = _run_case("all_bytes_" + case[0], golden, 1)
    want = ph.expected_all_bytes(case)
    assert got[0].shape == want.shape and got[0].dtype == want.dtype
    assert np.array_equal(got[0], want), [(ch, int((got[0][0, ch] != want[0, ch]).sum())) for ch in range(case[2]) if (got[0][0, ch] != want[0, ch]).any()]
    if case[1] == DT_INT8:               # both ends saturate (the lower one through the slope 3.3, channel 5); -128, an input, never comes out
        assert got[0].max() == 127 and got[0].min() == (-127 if case[2] > 5 else -21)


@pytest.mark.parametrize("case", ["u8_planes_49_bytes_batch2", "u8_planes_1_byte", "u8_plane_335_bytes", "u8_planes_aligned", "u8_planes_shared_slope"])
def test_uint8_plane_geometry(case, golden):
    """random bytes; planes that start at any byte address are cut at the 16-byte boundaries of their address"""
    _run_case(case, golden, 1)


def test_int8_batch_2_with_minus_128(golden):
    _run_case("i8_batch2_minus128", golden, 1)


def test_int8_padding_lanes_stay_zero_in_front_of_a_convolution(golden):
    """conv1x1 (8 -> 5) -> PReLU -> conv3x3 pad 1 (5 -> 7) at (2, 8, 5, 3): the second convolution reads the 11 lanes per pixel that the
    PReLU must have written as zero"""
    _run_case("i8_padding", golden, 1)


@pytest.mark.parametrize("case", ["i8_bottleneck", "u8_bottleneck"])
def test_bottleneck_through_the_c_abi(case, golden):
    """conv1x1 -> PReLU -> depthwise 3x3 -> PReLU -> conv1x1, + Eltwise SUM with the block's input, at (1, 8, 8, 8)"""
    _run_case(case, golden, 2)


def test_quarter_slope_is_a_relu_on_the_device():
    """0.25 widens to +0 in the reference, so PReLU(0.25) and ReLU with equal quantisation give equal bytes"""
    gp, gr, x = ph.quarter_and_relu_graphs(DT_INT8)
    a, names_p = _device(tm2.write_tm2(gp), x)
    b, names_r = _device(tm2.write_tm2(gr), x)
    assert names_p.count("prelu_i8") == 1 and names_r.count("prelu_i8") == 0
    assert (x < 0).any() and np.array_equal(a[0], b[0]) and (a[0][x < 0] == 0).all()


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_runs_the_bottleneck_as_one_hip_subgraph(ref, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, and the whole
    block -- both PReLUs included -- in ONE "HIP" subgraph.  The placement is asserted when the plugin in use is the one this tree's
    build() compiled (tengine_amd/lib/); the copy under oracle/_ref/ travels with a prebuilt reference and may be older (see
    tests/test_gpu_lut.py); the splitter itself is pinned in tests/test_prelu_cpu.py"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = ph.bottleneck_graph(dtype)
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
    assert real and real[0][0] == "HIP", pl
    if built_here:
        assert len(real) == 1 and real[0][1].count("PReLU") == 2, (tp.PLUGIN, pl)
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
