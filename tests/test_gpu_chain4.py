"""chain4.hip: producer conv -> depthwise 3x3 (stride 1) -> pointwise conv -> depthwise 3x3 (stride 1 | 2) as ONE launch -- a block owns a
spatial tile with all channels, the three intermediate maps only exist in LDS.  Bit-exact against the oracle and against the same graph
run as two pwdw launches on the device, for both producers (the network's first conv gathered from the NCHW input, a pointwise conv),
every border / partial-tile / clipped-region class, ragged channels and K, both depthwise formulas (batch 1 / batch > 1), and both kernel
instances (plain: hipGraph replay; coherent: direct dispatch)."""
import os

import numpy as np
import pytest

from oracle import oracle
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_INT8, DT_INT32, Graph

pytestmark = pytest.mark.gpu

NONE, RELU, RELU6 = -1, 0, 6


def chain_graph(seed, n, cin, h, w, c1, c2, s2, first=None, pad=1, acts=(RELU, RELU, RELU, RELU), c1_pad=None, mid_output=False, geoms=None):
    """producer (first = (k, stride, pad): a k x k conv on the NCHW graph input; None: a pointwise conv) -> dw1 (stride 1) -> pw2 ->
    dw2 (stride s2), biases on all four.  Every node's output scale follows helpers.pwdw_graph's rule, applied per layer:
    out = in * mean(weight scales) * 73 * sqrt(fan_in) * 73 / 60, weight scales uniform in [0.002, 0.02], bias in [-2000, 2000),
    input scale uniform in [0.01, 0.05], input bytes dense in [-127, 127].  `c1_pad`: pad of dw1 where it differs from dw2's;
    `mid_output`: dw1's output is a graph output as well; `geoms`: {"prod" | "dw1" | "dw2": per-axis geometry (helpers.conv_geom)} over
    the node's k / stride / pad."""
    from helpers import conv_geom, geom_out, geom_params
    rng = np.random.default_rng(seed)
    g = Graph(name="chain4_case")
    scale = float(np.float32(rng.uniform(0.01, 0.05)))
    t = g.add_input("data", [n, cin, h, w], DT_INT8, [scale], [0])
    x = rng.integers(-127, 128, size=(n, cin, h, w)).astype(np.int8)
    nodes = []

    def conv(name, out_name, cout, k, s, p, group, act):
        nonlocal t, scale, cin, h, w
        cg = cin // group
        G = conv_geom((geoms or {}).get(name), k, s, p)
        ws = [float(np.float32(v)) for v in rng.uniform(0.002, 0.02, size=cout)]
        ins = [t, g.add_const("w_" + name, rng.integers(-127, 128, size=(cout, cg, G["kh"], G["kw"])).astype(np.int8), DT_INT8, ws, [0] * cout),
               g.add_const("b_" + name, rng.integers(-2000, 2000, size=(cout,)).astype(np.int32), DT_INT32, [1.0], [0])]
        scale = float(np.float32(scale * np.mean(ws) * 73.0 * np.sqrt(cg * G["kh"] * G["kw"]) * 73.0 / 60.0))
        h, w = geom_out(h, w, G)
        t = g.add_tensor(out_name, [n, cout, h, w], DT_INT8, tm2.TT_VAR, None, [scale], [0])
        nodes.append(g.add_node(name, "Convolution", ins, [t], input_channel=cin, output_channel=cout, group=group, activation=act,
                                **geom_params(G)))
        cin = cout

    fk, fs, fp = first if first else (1, 1, 0)
    conv("prod", "m0", c1, fk, fs, fp, 1, acts[0])
    conv("dw1", "m1", c1, 3, 1, pad if c1_pad is None else c1_pad, c1, acts[1])
    conv("pw2", "m2", c2, 1, 1, 0, 1, acts[2])
    conv("dw2", "out", c2, 3, s2, pad, c2, acts[3])
    g.output_nodes = [nodes[1], nodes[3]] if mid_output else [nodes[3]]
    return g, x


def run(g, x, pin, direct=False, fuse_pwdw=None, keep=False):
    os.environ["TAMD_PIN"] = pin
    if fuse_pwdw is not None:
        os.environ["TAMD_FUSE_PWDW"] = str(fuse_pwdw)
    try:
        gr = capi.Graph(tm2.write_tm2(g), direct_dispatch=direct, keep_tensors=keep)
    finally:
        os.environ.pop("TAMD_PIN", None)
        os.environ.pop("TAMD_FUSE_PWDW", None)
    gr.set_input(x)
    outs = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    # kernel symbols of the AQL packets of a pass (the launch list plus the input / output layout launches); none: hipGraph replay
    packets = [capi.lib().tamd_graph_direct_packet_name(gr._h, i).decode() for i in range(gr.direct_packets())] if direct else []
    if keep:
        return outs, names, gr
    gr.close()
    return outs, names, packets


def is_chain(name):
    return name.split("_i8")[0] in ("chain4", "firstchain4")


# name -> (chain_graph arguments, pinned tiles, also under direct dispatch)
FIRST = (3, 2, 1)
CASES = {
    "first_20x22": (dict(seed=11, n=1, cin=3, h=20, w=22, c1=32, c2=64, s2=2, first=FIRST), ["2x2x256", "4x4x512", "7x7x512"], True),
    "first_b2_odd_ragged": (dict(seed=12, n=2, cin=3, h=37, w=41, c1=24, c2=40, s2=2, first=FIRST), [None], False),
    "first_b1_odd_ragged": (dict(seed=19, n=1, cin=3, h=37, w=41, c1=24, c2=40, s2=2, first=FIRST), [None], False),     # (batch 1: the other depthwise formula)
    "first_s1": (dict(seed=13, n=1, cin=3, h=30, w=30, c1=16, c2=32, s2=1, first=(3, 1, 1)), [None], False),
    "first_acts": (dict(seed=14, n=1, cin=3, h=26, w=18, c1=32, c2=64, s2=2, first=FIRST, acts=(NONE, RELU6, RELU, NONE)), [None], False),
    "pw_pairB_toy": (dict(seed=15, n=1, cin=64, h=12, w=10, c1=128, c2=128, s2=2), [None], True),
    "pw_ragged_pad0": (dict(seed=16, n=1, cin=40, h=9, w=13, c1=48, c2=72, s2=1, pad=0), [None], False),
    "pw_b3_two_k_steps": (dict(seed=17, n=3, cin=128, h=8, w=8, c1=128, c2=96, s2=2), [None], False),
    "pw_tile_larger_than_map": (dict(seed=18, n=1, cin=64, h=5, w=7, c1=64, c2=64, s2=1), ["7x7x256"], False),
}
_cache = {}


def case(name):
    """graph, input, the oracle's output and the device's two-launch output: computed once per case, shared, never modified"""
    if name not in _cache:
        g, x = chain_graph(**CASES[name][0])
        want = oracle.run_graph(g, x)[0]
        outs, names, _ = run(g, x, "chain4=0", fuse_pwdw=2)         # (=2: the pairs fuse at batch > 1 as well, without a race)
        assert len(names) == 2 and not any(is_chain(k) for k in names), names
        _cache[name] = (g, x, want, outs[0])
    return _cache[name]


PARITY = [(name, cfg, direct) for name, (_, cfgs, dd) in CASES.items() for cfg in cfgs for direct in ([False, True] if dd and cfg == cfgs[0] else [False])]


@pytest.mark.parametrize("name,cfg,direct", PARITY, ids=["%s-%s%s" % (n, c or "auto", "-direct" if d else "") for n, c, d in PARITY])
def test_parity(name, cfg, direct):
    g, x, want, two = case(name)
    # a degenerate graph cannot pass for parity
    assert len(np.unique(want)) >= 16 and np.count_nonzero(want == 0) < 0.8 * want.size
    outs, names, packets = run(g, x, "chain4=2" + (",chain4_cfg=" + cfg if cfg else ""), direct, fuse_pwdw=2)
    assert len(names) == 1 and is_chain(names[0]) and names[0].startswith("firstchain4" if CASES[name][0].get("first") else "chain4"), names
    if cfg:
        th, tw, threads = (int(v) for v in cfg.split("x"))
        oh, ow = want.shape[2], want.shape[3]
        assert names[0].endswith(",%dx%d,%d>" % (min(th, oh), min(tw, ow), threads)), names
    if direct:
        # exactly one packet is the coherent chain instance, no pair kernel beside it: no fall-back to hipGraph replay
        assert sum("chain4_i8_coh_kernel" in p for p in packets) == 1 and not any("pwdw_i8" in p for p in packets), packets
    got = outs[0].reshape(want.shape)
    bad = np.count_nonzero(got != want)
    assert bad == 0, "%s %s: %d / %d bytes differ from the oracle (max |d| %d)" % (name, names[0], bad, want.size, np.abs(got.astype(int) - want.astype(int)).max())
    assert np.array_equal(outs[0], two), "%s: differs from the two-launch plan on the device" % name


def inner_chain_graph(seed, n, hw):
    """a pointwise chain INSIDE a graph: 1x1 conv (16 -> 32) in front, the chain 32 -> 64 -> dw -> 64 -> dw, a 1x1 conv (64 -> 32) behind.
    Neither the chain's input nor its output is a graph input / output, so both live in the shared activation arena."""
    rng = np.random.default_rng(seed)
    g = Graph(name="chain4_inner")
    scale = float(np.float32(rng.uniform(0.01, 0.05)))
    t = g.add_input("data", [n, 16, hw, hw], DT_INT8, [scale], [0])
    x = rng.integers(-127, 128, size=(n, 16, hw, hw)).astype(np.int8)
    cin, h = 16, hw
    for name, cout, k, s, p, dw in (("pre", 32, 1, 1, 0, False), ("prod", 64, 1, 1, 0, False), ("dw1", 64, 3, 1, 1, True), ("pw2", 64, 1, 1, 0, False),
                                    ("dw2", 64, 3, 1, 1, True), ("post", 32, 1, 1, 0, False)):
        group = cin if dw else 1
        cg = cin // group
        ws = [float(np.float32(v)) for v in rng.uniform(0.002, 0.02, size=cout)]
        ins = [t, g.add_const("w_" + name, rng.integers(-127, 128, size=(cout, cg, k, k)).astype(np.int8), DT_INT8, ws, [0] * cout),
               g.add_const("b_" + name, rng.integers(-2000, 2000, size=(cout,)).astype(np.int32), DT_INT32, [1.0], [0])]
        scale = float(np.float32(scale * np.mean(ws) * 73.0 * np.sqrt(cg * k * k) * 73.0 / 60.0))
        h = (h - k + 2 * p) // s + 1
        t = g.add_tensor("t_" + name, [n, cout, h, h], DT_INT8, tm2.TT_VAR, None, [scale], [0])
        ni = g.add_node(name, "Convolution", ins, [t], kernel_h=k, kernel_w=k, stride_h=s, stride_w=s, dilation_h=1, dilation_w=1, input_channel=cin,
                        output_channel=cout, group=group, activation=RELU, pad_h0=p, pad_w0=p, pad_h1=p, pad_w1=p)
        cin = cout
    g.output_nodes = [ni]
    return g, x


def test_chain_inside_a_graph_with_shared_activation_buffers():
    """The chain's launch writes its output while it reads its input, at the FIRST node's position: with the activation arena on (the
    default) the two must not share memory.  The output (64 channels) is twice the input (32): laid over it, image k of the output covers
    images 2k and 2k + 1 of the input, so the blocks of image 3 would store over input images 6 and 7 -- which blocks 4704 .. 6271 of the
    launch read, more than 1500 blocks (more than can be resident at once) behind them."""
    g, x = inner_chain_graph(31, 8, 56)
    want = oracle.run_graph(g, x)[0]
    assert len(np.unique(want)) >= 16 and np.count_nonzero(want == 0) < 0.8 * want.size
    outs, names, _ = run(g, x, "chain4=2,chain4_cfg=2x2x256", fuse_pwdw=2)
    assert sum(is_chain(k) for k in names) == 1 and len(names) == 3, names
    two, names0, _ = run(g, x, "chain4=0", fuse_pwdw=2)
    assert not any(is_chain(k) for k in names0), names0          # (pairs, or at this batch depthwise + pointwise: the plan-time race's choice)
    assert np.array_equal(outs[0].reshape(want.shape), want)
    assert np.array_equal(outs[0], two[0])


def test_mobilenet_v1_batch1_with_both_chains_pinned():
    """chain4=2: the pointwise chain conv2_2/sep .. conv3_2/dw as well, whose input and output are both arena tensors"""
    if not _mbv1:
        g = models.build("mobilenet_v1", "int8", 1)
        x = models.synth_input(g, 7)
        _mbv1.update(g=g, x=x, want=oracle.run_graph(g, x)[0])
    outs, names, _ = run(_mbv1["g"], _mbv1["x"], "chain4=2")
    assert sum(is_chain(k) for k in names) == 2 and len(names) == 13, names
    assert np.array_equal(outs[0].reshape(_mbv1["want"].shape), _mbv1["want"])


def test_intermediates_of_a_chain_are_refused_by_read_tensor():
    g, x, want, _ = case("pw_tile_larger_than_map")
    outs, names, gr = run(g, x, "chain4=2", keep=True)
    try:
        assert len(names) == 1 and is_chain(names[0]), names
        assert np.array_equal(outs[0].reshape(want.shape), want)
        for nm in ("m0", "m1", "m2"):
            idx = [i for i, t in enumerate(g.tensors) if t.name == nm][0]
            with pytest.raises(capi.TamdError, match="TAMD_FUSE_PWDW=0"):
                gr.read_tensor(idx)
    finally:
        gr.close()


OUTSIDE = {
    "c1_144": dict(seed=21, n=1, cin=32, h=9, w=9, c1=144, c2=32, s2=1),
    "dw1_pad2": dict(seed=22, n=1, cin=32, h=9, w=9, c1=32, c2=32, s2=2, c1_pad=2),
    "mid_is_output": dict(seed=23, n=1, cin=32, h=9, w=9, c1=32, c2=32, s2=1, mid_output=True),
}


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_outside_the_limits_keeps_the_pairs(name):
    g, x = chain_graph(**OUTSIDE[name])
    want = oracle.run_graph(g, x)
    outs, names, _ = run(g, x, "chain4=2")
    _, names0, _ = run(g, x, "chain4=0")
    assert names == names0 and len(names) == 2 and not any(is_chain(k) for k in names), (names, names0)
    assert len(outs) == len(want)
    for got, ref in zip(outs, want):
        assert np.array_equal(got.reshape(ref.shape), ref)


def test_fuse_pwdw_0_disables_the_chain_and_the_pairs():
    g, x, want, _ = case("pw_tile_larger_than_map")
    outs, names, _ = run(g, x, "chain4=2", fuse_pwdw=0)
    assert len(names) == 4 and not any(k.split("_i8")[0] in ("chain4", "firstchain4", "pwdw", "firstdw") for k in names), names
    assert np.array_equal(outs[0].reshape(want.shape), want)


_mbv1 = {}


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "hipgraph"])
def test_mobilenet_v1_batch1_default_plan_runs_a_chain(direct):
    if not _mbv1:
        g = models.build("mobilenet_v1", "int8", 1)
        x = models.synth_input(g, 7)
        _mbv1.update(g=g, x=x, want=oracle.run_graph(g, x)[0])
    gr = capi.Graph(tm2.write_tm2(_mbv1["g"]), direct_dispatch=direct)
    try:
        gr.set_input(_mbv1["x"])
        got = gr.run()[0]
        names = [k["kernel"] for k in gr.profile(1)]
        assert np.array_equal(got.reshape(_mbv1["want"].shape), _mbv1["want"])
        assert len(names) < 15 and any(is_chain(k) for k in names), names
        if direct:
            assert gr.direct_packets() == gr.kernel_num(), (gr.direct_packets(), gr.kernel_num())     # no launch needed scratch: nothing fell back
    finally:
        gr.close()
