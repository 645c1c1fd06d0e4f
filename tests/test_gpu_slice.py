"""uint8 Slice on the device (csrc/slice_tables.cc + slice.hip): device bytes == the real reference library's bytes, from the committed
golden (tests/golden/slice_cases.npz, always) and from the reference itself (where oracle/_ref is built), through the C ABI with pooled
tensors (the default) and with keep_tensors = 1, twice per graph, and through the plugin.  The shapes are the smallest at which each
path of slice_u8 can go wrong:

  chan_requant            (1,12,3,5) axis 1 [5,12), 0.05/77 -> 0.031/12: an unaligned run, ragged ends, the byte map
  chan_batch2_identity    (2,8,3,5) [4,8), equal parameters: the image stride, the form without table
  full_range_raw_copy     (1,6,3,5) [0,6) between different scales: the reference's memcpy -- no requantisation
  full_range_end_clipped  .. the same with end = 100, clipped to the dimension
  end_negative, end_zero  end = -2 and end = 0: counted from the back
  batch_axis              (3,4,3,5) axis 0 [1,3): the image offset
  h_range                 (1,3,7,5) axis 2 [2,6): runs inside a plane
  w_range                 (1,3,4,37) axis 3 [3,36): 33-byte rows, chunks that cross rows, unaligned sources
  w_step2_even / _odd     (1,3,4,70) begin 0 / 1: two loads and byte permutes
  w_step2_odd_width       (1,3,4,71) begin 1: that path at a row's end
  h_step2                 (1,3,9,18) begin 1: strided rows, each copied whole
  c_step3                 (1,10,3,5) begin 1: strided planes
  w_step3                 (1,2,3,50): byte by byte
  blocks_ragged           (1,4,40,66) axis 3 step 2: several blocks, the last one partial
  chain                   (1,3,8,12) Slice(2, 1, step 2) -> Slice(3, 0, step 2), three different parameter pairs: one launch or two
  focus, csp              YOLOv5's Focus layer and a YOLOv4-tiny CSP block"""
import ctypes as C
import os

import numpy as np
import pytest

import lut_helpers as lh
import slice_op_helpers as so
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = so.gpu_cases()


@pytest.fixture(scope="module")
def golden():
    return so.golden()


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
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes.  Returns the launch
    list of the pooled run and the outputs"""
    g, x = CASES[case]()
    b = tm2.write_tm2(g)
    want = so.reference_outputs(ref_capi, g, x) if ref_capi.available() else None
    profs = []
    for keep in (False, True):
        got, prof = _device(b, x, keep_tensors=keep)
        profs.append([(k["node"], k["kernel"]) for k in prof])
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert so.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    assert profs[0] == profs[1]
    return profs[0], got


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


@pytest.mark.parametrize("case", sorted(so.SINGLE))
def test_slice_bytes_are_the_references(case, golden):
    """one slice_u8 launch under the node's name; the bytes are also the pick restated in numpy through tamd_slice_table (the input's
    own bytes for the raw copy)"""
    prof, got = _run_case(case, golden)
    assert prof == [("slice", "slice_u8")], prof
    g, x = CASES[case]()
    pick = so.numpy_slice(x, *so.SINGLE[case])
    q = lambda t: (g.tensors[t].scales[0], g.tensors[t].zero_points[0])
    want = pick if pick.shape == x.shape else capi.slice_table(*q(0), *q(1))[pick]
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize("case", ["w_step2_even", "w_step2_odd", "w_step2_odd_width", "blocks_ragged"])
def test_w_step2_path_gives_the_byte_by_byte_paths_bytes(case, golden):
    """TAMD_PIN=slice_w2=0 runs the generic gather on the same graph: the reference's bytes both ways"""
    slow = _pinned("slice_w2", 0, lambda: _run_case(case, golden))
    fast = _pinned("slice_w2", 1, lambda: _run_case(case, golden))
    assert slow[0] == fast[0] and np.array_equal(slow[1][0], fast[1][0])


def test_chain_of_two_slices_fused_and_as_two_launches(golden):
    """the default composes the two boxes and the two byte maps into ONE slice_u8 launch; TAMD_PIN=slice_chain=0 runs two: the same bytes"""
    fused, a = _run_case("chain", golden)
    two, b = _pinned("slice_chain", 0, lambda: _run_case("chain", golden))
    assert _pinned("slice_chain", 1, lambda: _run_case("chain", golden))[0] == fused
    assert fused == [("slice1+slice2", "slice_u8")], fused
    assert two == [("slice1", "slice_u8"), ("slice2", "slice_u8")], two
    assert np.array_equal(a[0], b[0])


def test_focus_layer(golden):
    """four chains -> Concat -> conv3x3: four fused launches by default, eight with TAMD_PIN=slice_chain=0, the reference's bytes both ways"""
    fused, a = _run_case("focus", golden)
    two, b = _pinned("slice_chain", 0, lambda: _run_case("focus", golden))
    slices = lambda prof: [n for n, k in prof if k == "slice_u8"]
    assert len(slices(fused)) == 4 and all("+" in n for n in slices(fused)), fused
    assert len(slices(two)) == 8 and not any("+" in n for n in slices(two)), two
    assert [k for _, k in fused if k != "slice_u8"] == [k for _, k in two if k != "slice_u8"]
    assert np.array_equal(a[0], b[0])


def test_csp_block(golden):
    """the route is one slice_u8 launch between the block's convolutions"""
    prof, _ = _run_case("csp", golden)
    assert [n for n, k in prof if k == "slice_u8"] == ["slice3"], prof


def test_every_case_is_run():
    assert set(so.SINGLE) | {"chain", "focus", "csp"} == set(CASES)


@pytest.mark.parametrize("case", ["csp", "focus"])
def test_plugin_runs_the_block_as_one_hip_subgraph(ref, case):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  One "HIP" subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the
    copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator
    table cannot know this operator (tests/test_gpu_shuffle.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = CASES[case]()
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
    assert any(dev == "HIP" for dev, _ in real), pl      # (Focus BEGINS with its Slices: under an older plugin the first subgraph is the CPU device's)
    if built_here:
        assert len(real) == 1 and real[0][0] == "HIP", (tp.PLUGIN, pl)
        assert "Slice" in real[0][1], pl
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
