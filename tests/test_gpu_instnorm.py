"""uint8 InstanceNorm on the device (csrc/node_rules.h: instancenorm_refusal; csrc/instnorm.hip): device bytes == the real reference
library's bytes, from the committed golden (tests/golden/instnorm_cases.npz, always) and from the reference itself (where oracle/_ref is
built), through the C ABI, twice per handle (the scratch maps are reused), in BOTH forms -- TAMD_PIN=instnorm_form=0: instnorm_stats_u8 +
chan_lut_u8; 1: instnorm_u8 -- with the kernels' names taken from the launch list and the two forms' bytes compared with each other, with
the ReLU folded and unfolded, and through the plugin.  Every byte is compared.  The shapes are the smallest at which the kernels can go
wrong (a wave per plane; a lane owns an aligned 16-byte chunk; a staged tile is 1024 floats):

  planes_1 / 3 / 4 / 5 / 130   (N,C,3,7): planes of 21 bytes at every misalignment; 130 = N 2 x C 65: more planes than lanes of a wave,
                               gamma / beta indexed by plane % C across the batch stride
  hw_1                         one byte per plane: var 0, every chunk ragged
  hw_15 / 16 / 17              below, at and above a chunk, planes 1 and 2 at odd addresses (C = 3): ragged head and tail
  hw_1024 / 1025 / 4099        one staged tile exactly; the tile boundary crossed by one element; five tiles, the fused remainder of
                               H * W % 4 = 3 elements behind them
  order_sensitive              planes of 4099 bytes from 236 .. 255: a wrong summation order changes hundreds of bytes here
  tiny_spread                  a constant plane (a = gamma / sqrt(eps): the fp64 sqrt and quotient alone) and planes with one other byte
  saturates_both_ends          bytes clamped at 0 and at 255
  gamma_zero_eps_1             gamma 0 (a constant output), a large negative gamma, eps 1, batch 2
  relu_folded / leaky_relu_folded   the ReLU composed into the map; with TAMD_PIN=instnorm_relu=0 a relu_u8 launch of its own: same bytes
  relu_not_alone               the tensor between is a graph output as well: not folded
  concat_and_second_reader     the output is read by a Concat (which copies: planes of 35 bytes) and by a ReLU
  generator_block (_batch2)    conv -> InstanceNorm -> ReLU -> conv whole, also through the plugin"""
import ctypes as C
import os

import numpy as np
import pytest

import instnorm_helpers as nh
from oracle import ref_capi
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = nh.gpu_cases()
FOLDING = ("relu_folded", "leaky_relu_folded", "generator_block", "generator_block_batch2")


@pytest.fixture(scope="module")
def golden():
    return nh.golden()


@pytest.fixture(scope="module")
def reference():
    """the reference's outputs of every case, computed once (where oracle/_ref is built)"""
    if not ref_capi.available():
        return {}
    return {case: nh.reference_outputs(ref_capi, *build()) for case, build in CASES.items()}


def _device(b, x):
    gr = capi.Graph(b)
    gr.set_input(x)
    out = gr.run()
    prof = gr.profile(1)
    again = gr.run()                                     # (the same handle: the scratch maps are written again before they are read)
    gr.close()
    for a, c in zip(out, again):
        assert np.array_equal(a, c)
    return out, [(k["node"], k["kernel"]) for k in prof]


def _pinned(pin, fn):
    old = os.environ.get("TAMD_PIN")
    os.environ["TAMD_PIN"] = pin
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["TAMD_PIN"]
        else:
            os.environ["TAMD_PIN"] = old


def _run_case(case, golden, want):
    """against the golden and, where it is built, the reference on the same bytes.  Returns the kernels of the InstanceNorm nodes' launches
    and of the ReLU nodes behind them, and the outputs"""
    g, x = CASES[case]()
    got, prof = _device(tm2.write_tm2(g), x)
    if want is not None:
        assert len(got) == len(want)
        for w, o in zip(want, got):
            assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
            assert np.array_equal(w, o), (case, int((w != o).sum()), w.size)
    assert nh.equals_golden(golden, case, got), (case, [o.shape for o in got])
    inorm = {n.name for n in g.nodes if n.op == "InstanceNorm"}
    relus = {n.name for n in g.nodes if n.op == "ReLU"}
    mine = [k for node, k in prof if set(node.split("+")) & inorm]
    return mine, [k for node, k in prof if node in relus], got


@pytest.mark.parametrize("case", sorted(CASES))
def test_both_forms_give_the_references_bytes(case, golden, reference):
    want = reference.get(case)
    outs = {}
    for form, kernels in ((0, ["instnorm_stats_u8", "chan_lut_u8"]), (1, ["instnorm_u8"])):
        mine, relus, outs[form] = _pinned("instnorm_form=%d" % form, lambda: _run_case(case, golden, want))
        assert mine == kernels, (case, form, mine)
        assert relus == ([] if case in FOLDING else ["relu_u8"] * sum(n.op == "ReLU" for n in CASES[case]()[0].nodes)), (case, relus)
    for a, b in zip(outs[0], outs[1]):
        assert a.dtype == b.dtype and np.array_equal(a, b), case     # the two forms, byte for byte
    if case in nh.SINGLE or case in ("order_sensitive", "tiny_spread"):
        g, x = CASES[case]()
        assert np.array_equal(outs[0][0], nh.restatement(g, x))      # .. and the host restatement


@pytest.mark.parametrize("case", FOLDING)
@pytest.mark.parametrize("form", [0, 1])
def test_relu_unfolded_gives_the_same_bytes(case, form, golden, reference):
    mine, relus, _ = _pinned("instnorm_form=%d,instnorm_relu=0" % form, lambda: _run_case(case, golden, reference.get(case)))
    assert mine == (["instnorm_stats_u8", "chan_lut_u8"] if form == 0 else ["instnorm_u8"]) and relus == ["relu_u8"], (mine, relus)


@pytest.mark.parametrize("case,kernels", [("generator_block", ["instnorm_u8"]), ("hw_1025", ["instnorm_u8"]), ("hw_4099", ["instnorm_stats_u8", "chan_lut_u8"])])
def test_the_default_form_follows_the_measured_threshold(case, kernels, golden, reference):
    """profiles/instnorm.txt: with nothing pinned one launch runs up to 4096 bytes a plane and two launches above; the ReLU is inside"""
    old = os.environ.pop("TAMD_PIN", None)
    try:
        mine, relus, _ = _run_case(case, golden, reference.get(case))
    finally:
        if old is not None:
            os.environ["TAMD_PIN"] = old
    assert mine == kernels and relus == [], (case, mine, relus)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("batch", [1, 2])
def test_plugin_runs_the_generator_block_as_one_hip_subgraph(ref, batch, form):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device.  One "HIP"
    subgraph is asserted when the plugin in use is the one this tree's build() compiled (tengine_amd/lib/): the copy under oracle/_ref/
    travels with a prebuilt reference and may have been compiled from an older hip_device.cc, whose operator table cannot know this
    operator (tests/test_gpu_shuffle.py states the rule)."""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = nh.generator_block(DT_UINT8, dims=(batch, 8, 9, 7))
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_UINT8)

    def run():
        rg = ref.RefGraph(b, ref.MODE_UINT8, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
        rg.set_input(x)
        rg.run()
        pl = tp.placement(rg)
        got = rg.outputs()
        rg.run()
        again = rg.outputs()
        rg.close()
        return pl, got, again
    pl, got, again = _pinned("instnorm_form=%d" % form, run)
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert any(dev == "HIP" for dev, _ in real), pl
    if built_here:
        assert len(real) == 1 and real[0][0] == "HIP", (tp.PLUGIN, pl)
        assert nh.REF_OP_NAME in real[0][1], pl
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
