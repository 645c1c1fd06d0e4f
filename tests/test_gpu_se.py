"""The channel-gate Eltwise on the device (csrc/chan_gate.hip: chan_gate_i8, chan_gate_u8 and their lut_ forms): device bytes == the
real reference library's bytes, from the committed golden (tests/golden/se_cases.npz, always) and from the reference itself (where
oracle/_ref is built), through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, and through the
plugin.  The launch list names the expected kernel exactly once per node.  The shapes are the smallest at which the kernels can go
wrong: all 65 536 byte pairs; int8 with 11 padding lanes, none, and a second quarter-full 16-lane group, at batch 2 (a gate indexed
without n shows); uint8 planes of 49 bytes (unaligned starts, chunks that span two planes), of two bytes, of 335 bytes (whole
chunks between two spanning ones, the second plane at an odd offset), and aligned ones."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import lut_helpers as lh
import se_helpers as sh
from oracle import ref_capi
from tengine_amd import tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sh.gpu_cases()
TAG = {DT_INT8: "i8", DT_UINT8: "u8"}
GATE_KERNELS = ["chan_gate_i8", "chan_gate_u8", "lut_chan_gate_i8", "lut_chan_gate_u8"]


@pytest.fixture(scope="module")
def golden():
    return sh.golden()


def _counts(names):
    return {k: names.count(k) for k in GATE_KERNELS + ["lut_u8", "eltwise_i8", "eltwise_u8"] if names.count(k)}


def _run_case(case, golden, expect):
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes; expect: {kernel: count}
    of the gate kernels, the byte map and the same-shape kernels in the launch list.  Returns the outputs of the pooled run"""
    dtype, build = CASES[case]
    g, xs = build()
    for i, x in enumerate(xs):
        assert np.array_equal(golden["%s__in%d" % (case, i)], x)
    b = tm2.write_tm2(g)
    want = sh.reference_outputs(ref_capi, g, xs, dtype) if ref_capi.available() else None
    first = None
    for keep in (False, True):
        got, names, _ = sh.device_outputs(b, xs, keep_tensors=keep)
        assert _counts(names) == expect, names
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert sh.equals_golden(golden, case, got), (case, keep, [int((golden["%s__out%d" % (case, i)] != o).sum()) for i, o in enumerate(got)])
        first = first or got
    return first


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("typ", sorted(sh.TYPES))
def test_every_byte_pair(dtype, typ, golden):
    """x (1, 256, 16, 16), every channel all 256 values, gate byte c in channel c: the device equals the reference AND the numpy
    restatement on all 65 536 pairs; both ends of the clamp are reached, and -128, an input of both operands, never comes out"""
    got = _run_case("pairs_%s_%s" % (TAG[dtype], typ), golden, {"chan_gate_" + TAG[dtype]: 1})[0]
    xs = sh.all_pairs_inputs(dtype)
    qx, qg, qo = sh.QUANT[dtype]
    want = sh.restate(dtype, typ, xs[0], xs[1], qx, qg, qo[typ])
    assert np.array_equal(got, want), [(c, int((got[0, c] != want[0, c]).sum())) for c in range(256) if (got[0, c] != want[0, c]).any()][:8]
    assert (got.min(), got.max()) == ((-127, 127) if dtype == DT_INT8 else (0, 255))


@pytest.mark.parametrize("case", ["i8_lanes_c5", "i8_lanes_c16", "i8_lanes_c20", "i8_two_pixels"])
def test_int8_lane_geometry(case, golden):
    """random bytes with -128 in both operands, batch 2: 11 padding lanes; none; a second, quarter-full group; one group of two pixels"""
    _run_case(case, golden, {"chan_gate_i8": 1})


@pytest.mark.parametrize("iters", [1, 2, 4])
def test_int8_lanes_that_walk_several_pixels(iters, golden, tmp_path):
    """(2, 480, 5, 5): 30 channel groups, so a block iteration is 8 pixels and the 25 pixels of an image are a ragged walk.  The launcher
    lets a lane walk 2 or 4 pixels only on tensors far larger than a test may be, so a fresh child process pins the count
    (TAMD_PIN=gate_iters=N): the same bytes, the reference's, for every count"""
    case = "i8_walk_c480"
    want = _run_case(case, golden, {"chan_gate_i8": 1})
    out = str(tmp_path / "walk.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import se_helpers as sh; sh.child_main(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), case, out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TAMD_PIN="gate_iters=%d" % iters), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert _counts([str(k) for k in z["names"]]) == {"chan_gate_i8": 1} and np.array_equal(z["out0"], want[0])


def test_int8_padding_lanes_stay_zero_in_front_of_a_convolution(golden):
    """conv1x1 (8 -> 5) -> SUM with a gate -> conv3x3 pad 1 (5 -> 7) at (2, 8, 5, 3): the second convolution reads the 11 lanes per pixel
    that the gate kernel must have written as zero"""
    _run_case("i8_padding", golden, {"chan_gate_i8": 1})


@pytest.mark.parametrize("case", ["u8_planes_49_bytes_batch2", "u8_planes_2_bytes", "u8_planes_335_bytes", "u8_planes_aligned"])
def test_uint8_plane_geometry(case, golden):
    """random bytes; planes start at any byte address: a lane's aligned 16 bytes lie in one plane or in two (49- and 335-byte planes), the
    tensor's last chunk is ragged (98 and 670 bytes), and planes of fewer than 16 bytes take the byte-per-lane form"""
    _run_case(case, golden, {"chan_gate_u8": 1})


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("typ", sorted(sh.TYPES))
def test_gate_listed_first(dtype, typ, golden):
    """batch 1: x op gate whichever is listed first -- SUB is x - gate -- and the output has x's dims"""
    case = "%s_gate_first_%s" % (TAG[dtype], typ)
    got = _run_case(case, golden, {"chan_gate_" + TAG[dtype]: 1})[0]
    _, xs = CASES[case][1]()
    qx, qg, qo = sh.QUANT[dtype]
    assert got.shape == xs[0].shape and np.array_equal(got, sh.restate(dtype, typ, xs[0], xs[1], qx, qg, qo[typ]))


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_se_block_folded_two_launches_and_split(dtype, golden, tmp_path):
    """conv -> GAP -> conv -> ReLU -> conv -> Sigmoid -> PROD -> conv at (2, 8, 6, 6), reduce 4.  Default: the Sigmoid's byte map runs
    inside the gate's launch (lut_chan_gate_* once, lut_u8 never).  A fresh child process with TAMD_PIN=gate_lut=0: lut_u8 and
    chan_gate_* once each, the same bytes.  split_batch = 2 (two half-batch graphs): the same bytes"""
    case = TAG[dtype] + "_se_block"
    folded = _run_case(case, golden, {"lut_chan_gate_" + TAG[dtype]: 1})
    out = str(tmp_path / "two.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import se_helpers as sh; sh.child_main(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), case, out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TAMD_PIN="gate_lut=0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert _counts([str(k) for k in z["names"]]) == {"lut_u8": 1, "chan_gate_" + TAG[dtype]: 1}, z["names"]
    assert np.array_equal(z["out0"], folded[0])
    g, xs = CASES[case][1]()
    halves, _, n = sh.device_outputs(tm2.write_tm2(g), xs, split_batch=2)
    assert n == 2 and np.array_equal(halves[0], folded[0])


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_sigmoid_with_a_second_reader_is_not_folded(dtype, golden):
    """the Sigmoid's output is also a graph output: it is written by lut_u8, the gate reads it, and both outputs are the reference's"""
    got = _run_case(TAG[dtype] + "_multi_reader", golden, {"lut_u8": 1, "chan_gate_" + TAG[dtype]: 1})
    assert len(got) == 2 and got[1].shape == (2, 8, 1, 1)


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_plugin_runs_the_se_block_as_one_hip_subgraph(ref, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, and the whole
    block -- the gate included -- in ONE "HIP" subgraph.  The placement is asserted when the plugin in use is the one this tree's
    build() compiled (tengine_amd/lib/); the copy under oracle/_ref/ travels with a prebuilt reference and may be older (see
    tests/test_gpu_lut.py); the splitter itself is pinned in tests/test_se_cpu.py"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = sh.se_block_graph(dtype)
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
        assert len(real) == 1 and real[0][1].count("Eltwise") == 1, (tp.PLUGIN, pl)
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
