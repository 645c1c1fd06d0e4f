"""Quantised Split and ShuffleChannel on the device (csrc/chanmap_tables.cc + chanmap.hip): device bytes == the real reference
library's bytes, from the committed golden (tests/golden/shuffle_cases.npz, always) and from the reference itself (where oracle/_ref is
built), through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice per graph, and through the plugin.  The
shapes are the smallest at which the kernels can go wrong: one vector with padding lanes, sources that cross the vector boundary, an
image stride, the real stage-2 width, several blocks with a ragged last one, identity maps, unaligned and aligned Split outputs, Split
outputs as views, odd uint8 planes, and the ShuffleNet-v2 units with Concat + ShuffleChannel as one launch and as two."""
import ctypes as C
import os

import numpy as np
import pytest

import lut_helpers as lh
import shuffle_helpers as sh
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sh.gpu_cases()
KERNEL = {DT_INT8: "chan_map_i8", DT_UINT8: "chan_map_u8"}


@pytest.fixture(scope="module")
def golden():
    return sh.golden()


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
    list of the pooled run"""
    dtype, build = CASES[case]
    g, x = build()
    b = tm2.write_tm2(g)
    want = sh.reference_outputs(ref_capi, g, x, dtype) if ref_capi.available() else None
    shapes = []                                          # of the reference's outputs, as the golden holds them
    for i in range(int(golden[case + "__n"])):
        k = "%s__shape%d" % (case, i)
        shapes.append(tuple(golden[k]) if k in golden.files else golden["%s__out%d" % (case, i)].shape)
    profs = []
    for keep in (False, True):
        got, prof = _device(b, x, keep_tensors=keep)
        got = [sh.in_reference_shape(o, s) for o, s in zip(got, shapes)]
        profs.append([(k["node"], k["kernel"]) for k in prof])
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert sh.equals_golden(golden, case, got), (case, keep, [o.shape for o in got])
    assert profs[0] == profs[1]
    return profs[0]


def _movers(prof, dtype=DT_INT8):
    """the nodes of the channel-map launches (chan_map_i8 and its group-2 form chan_map_i8_g2; chan_map_u8)"""
    return [node for node, kernel in prof if kernel.startswith(KERNEL[dtype])]


SHUFFLES = sorted(c for c in CASES if "_shuffle_" in c and "cat" not in c and "padding" not in c)


@pytest.mark.parametrize("case", SHUFFLES)
def test_shuffle_channel_bytes_are_the_references(case, golden):
    """one launch per node, by name; -128 stays -128 and the output's own scale is not read"""
    prof = _run_case(case, golden)
    assert _movers(prof, CASES[case][0]) == ["shuffle"], prof


def test_shuffle_is_the_reshape_transpose_on_the_device():
    """.. and the bytes are the input's own, moved: no golden and no reference in between"""
    for dtype, dims, group in ((DT_INT8, (2, 20, 3, 2), 2), (DT_UINT8, (2, 12, 3, 5), 3), (DT_INT8, (1, 116, 4, 4), 2)):
        g, x = sh.shuffle_graph(dtype, dims, group, force=-128 if dtype == DT_INT8 else None)
        got, _ = _device(tm2.write_tm2(g), x)
        n, c, h, w = dims
        assert np.array_equal(got[0], x.reshape(n, group, c // group, h, w).transpose(0, 2, 1, 3, 4).reshape(dims))
        assert np.array_equal(got[0], x[:, capi.shuffle_sources(c, group)])


@pytest.mark.parametrize("case", ["i8_split_unaligned", "i8_split_one_aligned_batch2", "i8_split_scale_differs_minus128"])
def test_int8_split_bytes_are_the_references(case, golden):
    """data -> Split -> Concat(reversed): one chan_map_i8 launch per output tensor, under the Split's name"""
    prof = _run_case(case, golden)
    g, _ = CASES[case][1]()
    outputs = len([n for n in g.nodes if n.op == "Split"][0].outputs)
    assert _movers(prof) == ["split"] * outputs, prof


def test_int8_split_outputs_as_views_have_no_launch(golden):
    """[16, 16] of a convolution's 32 channels, read by a 1x1 and a 3x3 convolution: channel slices of the pixels as they lie"""
    prof = _run_case("i8_split_views", golden)
    assert _movers(prof) == [] and not any("split" in node for node, _ in prof), prof


def test_int8_shuffle_padding_lanes_are_zero_for_the_next_convolution(golden):
    prof = _run_case("i8_shuffle_padding", golden)
    assert len(_movers(prof)) == 1, prof


def _pinned(value, fn, key="cat_shuffle"):
    old = os.environ.get("TAMD_PIN")
    os.environ["TAMD_PIN"] = "%s=%d" % (key, value)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["TAMD_PIN"]
        else:
            os.environ["TAMD_PIN"] = old


@pytest.mark.parametrize("unit", sorted(sh.UNITS))
def test_int8_units_fused_and_two_step(unit, golden):
    """Concat -> ShuffleChannel as ONE chan_map_i8 launch (the default) and as two steps (TAMD_PIN=cat_shuffle=0): the same bytes -- the
    reference's -- in both; fused: no concat_copy_i8 and exactly one chan_map_i8 for the pair; two steps: the Concat's launches of
    before plus one for the ShuffleChannel"""
    case = "i8_" + unit
    g, _ = CASES[case][1]()
    pairs = sum(n.op == "ShuffleChannel" for n in g.nodes)
    fused = _run_case(case, golden)
    two = _pinned(0, lambda: _run_case(case, golden))
    assert _pinned(1, lambda: _run_case(case, golden)) == fused
    kernels = lambda prof: [k for _, k in prof]
    assert "concat_copy_i8" not in kernels(fused), fused
    assert len([n for n in _movers(fused) if "+" in n and "shuffle" in n and "cat" in n]) == pairs, fused
    assert not any(n.startswith("shuffle") for n in _movers(fused)), fused
    assert len([n for n in _movers(two) if n.startswith("shuffle")]) == pairs and not any("+" in n for n in _movers(two)), two
    assert kernels(two).count("concat_copy_i8") >= pairs    # (the Split's pass-through half is never written in place)
    splits = lambda prof: [n for n in _movers(prof) if n.startswith("split")]
    assert splits(two) == splits(fused)


@pytest.mark.parametrize("unit", sorted(sh.UNITS))
def test_group2_interleave_form_gives_the_table_forms_bytes(unit, golden):
    """group 2 over two halves of equal width runs as chan_map_i8_g2 (two 8-byte loads, four byte permutes, one store) where the halves
    lie 8-byte aligned; TAMD_PIN=chan_map_g2=0 runs the table form on the same graph: both are the reference's bytes, and the interleave
    form is taken exactly where its conditions hold"""
    case = "i8_" + unit
    g, _ = CASES[case][1]()
    table = _pinned(0, lambda: _run_case(case, golden), "chan_map_g2")
    inter = _pinned(1, lambda: _run_case(case, golden), "chan_map_g2")
    assert [n for n, _ in table] == [n for n, _ in inter]
    assert not any(k == "chan_map_i8_g2" for _, k in table), table
    want = 0
    for n in g.nodes:                                    # the pairs whose Concat has two inputs of equal width in front of a group-2 shuffle
        if n.op == "ShuffleChannel" and n.params["group"] == 2:
            cat = g.producer(n.inputs[0])
            want += cat.op == "Concat" and len(cat.inputs) == 2 and g.tensors[cat.inputs[0]].dims == g.tensors[cat.inputs[1]].dims
    assert [k for _, k in inter].count("chan_map_i8_g2") == want, inter


def test_group2_interleave_form_on_one_tensor():
    """ShuffleChannel(2) of one tensor whose half width is a multiple of 8: the two halves are slices of the same pixels; -128 stays"""
    for dims in ((2, 16, 3, 5), (1, 48, 4, 4)):
        g, x = sh.shuffle_graph(DT_INT8, dims, 2, force=-128)
        b = tm2.write_tm2(g)
        inter, pi = _pinned(1, lambda: _device(b, x), "chan_map_g2")
        table, pt = _pinned(0, lambda: _device(b, x), "chan_map_g2")
        assert [k["kernel"] for k in pi] == ["chan_map_i8_g2"] and [k["kernel"] for k in pt] == ["chan_map_i8"]
        n, c, h, w = dims
        assert np.array_equal(inter[0], table[0]) and np.array_equal(inter[0], x.reshape(n, 2, c // 2, h, w).transpose(0, 2, 1, 3, 4).reshape(dims))


@pytest.mark.parametrize("case", ["u8_split_requant_and_identity", "u8_unit_half6"])
def test_uint8_split_and_unit(case, golden):
    """one chan_map_u8 launch per Split output and per ShuffleChannel; one Split output is requantised (0.05 / 77 -> 0.031 / 12), the
    other carries the input's parameters and skips the map"""
    prof = _run_case(case, golden)
    g, _ = CASES[case][1]()
    want = sum(len(n.outputs) for n in g.nodes if n.op == "Split") + sum(n.op == "ShuffleChannel" for n in g.nodes)
    assert len(_movers(prof, DT_UINT8)) == want, prof


def test_every_case_is_run():
    mine = set(SHUFFLES) | {"i8_split_unaligned", "i8_split_one_aligned_batch2", "i8_split_scale_differs_minus128", "i8_split_views", "i8_shuffle_padding",
                            "u8_split_requant_and_identity", "u8_unit_half6"} | {"i8_" + u for u in sh.UNITS}
    assert mine == set(CASES)


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8])
def test_plugin_runs_the_unit_as_one_hip_subgraph(ref, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, whatever the
    placement.  One "HIP" subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the
    copy under oracle/_ref/ travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator
    table cannot know these operators (tests/test_gpu_interp.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = sh.basic_unit_graph(dtype, 6)
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
