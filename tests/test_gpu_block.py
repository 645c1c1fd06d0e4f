"""block_i8.hip: an identity bottleneck block -- conv 1x1 -> conv 3x3 (stride 1, pad 1) -> conv 1x1 -> Eltwise SUM with the block's input
[-> ReLU] -- as ONE launch (opt-in: TAMD_FUSE_BLOCK=1), neither intermediate map leaving LDS.  Bit-exact against the oracle, whose
four-node result is what the reference computes (both intermediate int8 roundings and its eltwise formula included), and against the
same graph run as three launches on the device; the shapes the first version does not take stay three launches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from block_helpers import block_graph, requantised_bias, tensor_index
from oracle import oracle
from tengine_amd import capi, models, tm2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(g, x, fuse, **kw):
    """fuse: "1" / "0" sets TAMD_FUSE_BLOCK around the prerun, None leaves it unset"""
    old = os.environ.pop("TAMD_FUSE_BLOCK", None)
    if fuse is not None:
        os.environ["TAMD_FUSE_BLOCK"] = str(fuse)
    try:
        gr = capi.Graph(tm2.write_tm2(g), **kw)
    finally:
        os.environ.pop("TAMD_FUSE_BLOCK", None)
        if old is not None:
            os.environ["TAMD_FUSE_BLOCK"] = old
    gr.set_input(x)
    outs = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    return outs, names, gr


def differing(got, want):
    assert len(got) == len(want)
    return sum(int(np.count_nonzero(o.reshape(w.shape) != w)) for o, w in zip(got, want))


# id -> block_graph arguments
CASES = {
    "res2_n2_256x56x56_mid64": dict(seed=1, n=2, c=256, h=56, w=56, mid=64),
    "partial_tiles_3x256x13x9": dict(seed=2, n=3, c=256, h=13, w=9, mid=64),
    "smaller_than_a_tile_1x64x3x5": dict(seed=3, n=1, c=64, h=3, w=5, mid=64),
    "mid16_c64": dict(seed=4, n=2, c=64, h=17, w=11, mid=16),
    "mid32_c128": dict(seed=5, n=2, c=128, h=16, w=24, mid=32),
    "c128_mid64_batch1": dict(seed=6, n=1, c=128, h=20, w=20, mid=64),
    "no_bias": dict(seed=7, n=2, c=64, h=12, w=12, mid=32, bias=False),
    "no_relu_after_the_add": dict(seed=8, n=2, c=128, h=10, w=15, mid=64, relu=False),
    "eltwise_reads_conv_first": dict(seed=9, n=2, c=64, h=9, w=9, mid=64, conv_first=True),
    "negative_values_through_both_requantisations": dict(seed=10, n=2, c=128, h=14, w=14, mid=64, act_lead=-1, act_a=-1),
    "relu_requantises": dict(seed=11, n=1, c=64, h=11, w=8, mid=32, relu_scale=0.8),        # the tail's general form (no folded sum)
    "mid48_c96_batch5": dict(seed=12, n=5, c=96, h=8, w=8, mid=48),                         # ragged middle tile, C not a power of two
}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_block_matches_the_oracle_and_three_launches(case):
    g, x = block_graph(**CASES[case])
    want = oracle.run_graph(g, x)
    got, names, gr = run(g, x, "1")
    gr.close()
    bad = differing(got, want)
    print(case, "fused:", names, "differing bytes:", bad)
    assert names[1:] == ["block_i8"] and len(names) == 2, names          # the leading conv, then the block as ONE launch
    assert bad == 0, "%s: %d / %d bytes differ" % (case, bad, want[0].size)
    assert len(np.unique(want[0])) >= 5
    off, names0, gr0 = run(g, x, "0")
    gr0.close()
    assert len(names0) == 4 and "block_i8" not in names0, names0
    assert differing(off, got) == 0


def test_out_of_image_halo_is_zero_not_the_requantised_bias():
    """the 3x3's padding pads branch2a's OUTPUT with zeros.  branch2a's biases here are large and positive, so a map position computed
    from an all-zero input (what a kernel gets that runs branch2a on a zero-filled halo) would hold relu(requant(bias)) > 0"""
    g, x = block_graph(seed=21, n=2, c=64, h=9, w=10, mid=32, bias_a_range=(3000, 20000))
    q = requantised_bias(g, "mid1")
    assert np.count_nonzero(q > 0) * 2 >= q.size, q
    want = oracle.run_graph(g, x)
    got, names, gr = run(g, x, "1")
    gr.close()
    assert "block_i8" in names, names
    assert differing(got, want) == 0
    assert len(np.unique(want[0])) >= 5


REFUSED = {
    "stride2_branch2a": dict(seed=31, n=2, c=64, h=12, w=12, mid=32, stride_a=2),
    "mid128": dict(seed=32, n=1, c=256, h=10, w=10, mid=128),
    "dilation2": dict(seed=33, n=2, c=64, h=12, w=12, mid=32, dil_b=2),
    "residual_from_a_projection": dict(seed=34, n=2, c=64, h=12, w=12, mid=32, projection=True),
    "branch2a_output_consumed_twice": dict(seed=35, n=2, c=64, h=12, w=12, mid=32, a_twice=True),
    "branch2b_output_is_a_graph_output": dict(seed=36, n=2, c=64, h=12, w=12, mid=32, b_is_output=True),
}


@pytest.mark.parametrize("case", list(REFUSED), ids=list(REFUSED))
def test_shapes_outside_the_first_version_stay_three_launches(case, monkeypatch):
    """switch on: the launch list of the switch-off run, name for name -- every convolution of the block its own launch, as today.
    (TAMD_AUTOTUNE=0: the kernel lists of two separate preruns are compared, so no plan-time race may pick them.)"""
    monkeypatch.setenv("TAMD_AUTOTUNE", "0")
    g, x = block_graph(**REFUSED[case])
    want = oracle.run_graph(g, x)
    got, names, gr = run(g, x, "1")
    nodes = [k["node"] for k in gr.profile(1)]
    gr.close()
    off, names_off, gr0 = run(g, x, "0")
    nodes_off = [k["node"] for k in gr0.profile(1)]
    gr0.close()
    print(case, "on:", list(zip(nodes, names)))
    assert "block_i8" not in names, names
    assert names == names_off and nodes == nodes_off, (names, names_off)
    convs = ("mid1", "mid2", "branch2c")                                  # each of the block's three convs is a launch of its own
    for conv in convs:
        assert [len(set(n.split("+")) & set(convs)) for n in nodes if conv in n.split("+")] == [1], nodes
    assert differing(got, want) == 0 and differing(off, want) == 0


def test_both_intermediate_maps_are_refused_when_fused():
    g, x = block_graph(seed=41, n=2, c=64, h=12, w=12, mid=32)
    want = oracle.run_graph(g, x)
    got, names, gr = run(g, x, "1", keep_tensors=True)
    assert "block_i8" in names, names
    for t in ("mid1", "mid2"):
        with pytest.raises(capi.TamdError, match="fused"):
            gr.read_tensor(tensor_index(g, t))
    out = gr.read_tensor(tensor_index(g, "out"))
    gr.close()
    assert np.array_equal(out.reshape(want[0].shape), want[0])
    assert differing(got, want) == 0


def test_resnet50_batch2_fuses_res2b_and_res2c_only_when_asked(monkeypatch):
    """switch on: two launches of block_i8 (res2b, res2c), four launches fewer; switch unset: the plan of the switch-off run, name for
    name.  (TAMD_AUTOTUNE=0: the kernel lists of three separate preruns are compared, so no plan-time race may pick them.)"""
    monkeypatch.setenv("TAMD_AUTOTUNE", "0")
    g = models.build("resnet50", "int8", 2, device_only=True)
    x = models.synth_input(g, 31)
    want = oracle.run_graph(g, x)
    on, names_on, gr = run(g, x, "1")
    nodes_on = [k["node"] for k in gr.profile(1)]
    gr.close()
    off, names_off, gr = run(g, x, "0")
    gr.close()
    unset, names_unset, gr = run(g, x, None)
    gr.close()
    print("on:", names_on)
    assert names_on.count("block_i8") == 2, names_on
    fused = [n for n, k in zip(nodes_on, names_on) if k == "block_i8"]
    assert fused == ["res2b_branch2a+res2b_branch2b+res2b_branch2c", "res2c_branch2a+res2c_branch2b+res2c_branch2c"], fused
    assert len(names_on) == len(names_off) - 4, (len(names_on), len(names_off))
    assert "block_i8" not in names_off and "block_i8" not in names_unset
    assert names_unset == names_off
    assert differing(on, want) == 0 and differing(off, want) == 0 and differing(unset, want) == 0
    assert len(np.unique(want[0])) >= 5


def test_resnet50_batch32_in_the_shipped_form(ref):
    """direct dispatch, the default split rule (two half-batch graphs side by side), the switch on: the real reference's bytes through the
    blocking run and through the resident upload / launch / sync / download path"""
    g = models.build("resnet50", "int8", 32, device_only=True)
    x = models.synth_input(g, 22)
    tmb = tm2.write_tm2(g)
    want = ref.run_model(tmb, x, ref.MODE_INT8, min(os.cpu_count() or 1, 64))
    got, names, gr = run(g, x, "1", direct_dispatch=True)
    try:
        assert gr.halves() == 2
        assert gr.direct_packets() > 0
        assert "block_i8" in names, names
        assert differing(got, want) == 0
        gr.upload()
        for _ in range(3):
            gr.launch()
        gr.sync()
        assert differing(gr.download(), want) == 0
        assert differing(gr.run(), want) == 0
    finally:
        gr.close()
    assert len(np.unique(want[0])) >= 5


PLUGIN_SCRIPT = r'''
import ctypes as C, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import test_plugin_dropin as tp
from oracle import ref_capi as ref
from tengine_amd import models, tm2
tp._load_plugin(ref)
g = models.build("resnet50", "int8", 2)
x = models.synth_input(g, 8)
b = tm2.write_tm2(g)
want = ref.run_model(b, x, ref.MODE_INT8, 4)
rg = ref.RefGraph(b, ref.MODE_INT8, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 1))      # profile = 1
rg.set_input(x)
rg.run()
tp.assert_all_on_hip(rg)
got = rg.outputs()
rg.close()
print("SAME", bool(len(want) == len(got) and all(np.array_equal(w, o) for w, o in zip(want, got))))
'''


def test_the_plugin_gets_the_fusion_through_the_library(ref):
    """ResNet-50 int8 batch 2 through the reference's own API on device "HIP", in a fresh process with the switch set: the reference CPU
    device's bytes, and block_i8 in the per-launch table the profile option prints at postrun"""
    import test_plugin_dropin as tp
    if not os.path.exists(tp.PLUGIN):
        pytest.skip("plugin not built (needs the reference headers once)")
    env = dict(os.environ)
    env["TAMD_FUSE_BLOCK"] = "1"
    r = subprocess.run([sys.executable, "-c", PLUGIN_SCRIPT % (ROOT, os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "SAME True" in r.stdout, r.stdout
    assert "block_i8" in r.stderr, r.stderr[-3000:]
