"""Quantised nearest Interp on the device (csrc/interp_tables.cc + interp.hip): device bytes == the real reference library's bytes,
from the committed golden (tests/golden/interp_nearest_cases.npz, always) and from the reference itself (where oracle/_ref is built),
through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, and through the plugin.  The shapes are
the smallest at which the kernels can go wrong: int8 padding lanes in front of a convolution that reads them, per-axis / non-integer /
shrinking scales, sizes-only parameters, odd uint8 planes (unaligned rows), several blocks with a ragged last one, concat in place
and by copy."""
import ctypes as C
import os

import numpy as np
import pytest

import interp_helpers as ih
import lut_helpers as lh
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ih.gpu_cases()
KERNEL = {DT_INT8: "interp_nearest_i8", DT_UINT8: "interp_nearest_u8"}


@pytest.fixture(scope="module")
def golden():
    return ih.golden()


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
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes; one launch per Interp node,
    by name.  Returns the launch list of the pooled run"""
    dtype, build = CASES[case]
    g, x = build()
    b = tm2.write_tm2(g)
    want = ih.reference_outputs(ref_capi, g, x, dtype) if ref_capi.available() else None
    interps = sum(n.op == "Interp" for n in g.nodes)
    profs = []
    for keep in (False, True):
        got, prof = _device(b, x, keep_tensors=keep)
        profs.append(prof)
        names = [k["kernel"] for k in prof]
        assert names.count(KERNEL[dtype]) == interps and not any(n.startswith("upsample") for n in names), names
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert ih.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    return profs[0]


PLAIN = sorted(c for c in CASES if "concat" not in c and "identity" not in c)


@pytest.mark.parametrize("case", PLAIN)
def test_device_bytes_are_the_references(case, golden):
    _run_case(case, golden)


def test_int8_concat_in_place(golden):
    """a x2 Interp of 16 channels whose only reader is a channel concat at its own scale writes into the concat's buffer: no copy launch"""
    prof = _run_case("i8_concat_in_place", golden)
    assert not any(k["kernel"] == "concat_copy_i8" for k in prof), prof


def test_int8_concat_fallback(golden):
    """8 channels: no slice of 16 -- the Interp keeps its own buffer and the concat copies; prerun succeeds"""
    prof = _run_case("i8_concat_fallback", golden)
    assert any(k["kernel"] == "concat_copy_i8" for k in prof), prof


def test_uint8_concat_in_place_at_an_odd_plane_start(golden):
    """the Interp's five 81-byte planes start at byte 243 of the concat's image: no row and no plane is aligned, no copy launch"""
    prof = _run_case("u8_concat_in_place_odd_start", golden)
    assert not any(k["kernel"].startswith("concat") for k in prof), prof


def test_uint8_identity_path_by_bytes(golden):
    """equal quantisation on both sides: the kernel skips the lookup; the bytes are the input's own, moved (and the reference's)"""
    _run_case("u8_identity", golden)
    g, x = CASES["u8_identity"][1]()
    got, _ = _device(tm2.write_tm2(g), x)
    iy, ix = capi.interp_indices(5, 7, lh.f32(1.5)), capi.interp_indices(7, 21, lh.f32(3.0))
    assert np.array_equal(got[0], x[:, :, iy][:, :, :, ix])


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8])
def test_plugin_runs_the_neck_as_one_hip_subgraph(ref, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  WHERE the node lands is the splitter's decision and is pinned where the plugin is always built from this tree's source
    (tests/test_interp_cpu.py).  It is asserted here too -- one "HIP" subgraph -- when the plugin in use is the one this tree's build()
    compiled (tengine_amd/lib/).  The copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older
    hip_device.cc, whose operator table cannot know Interp: with such a binary the node is a CPU node between device subgraphs, the
    bytes must still be the reference's, and nothing in this tree can change where that binary puts it."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = ih.neck_graph(dtype)
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
        assert len(real) == 1, (tp.PLUGIN, pl)
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
