"""pwdw.hip: the kernels rebuild their argument struct from one fetch of the argument segment (pwdw_fetch_args) instead of taking the
fields from the by-value argument.  Every case is byte-equal to the oracle (tests/test_oracle_vs_reference.py pins it to the real
reference) and runs twice: as hipGraph replay (the plain instances) and directly dispatched (the coherent instances).

One case per tail, producer and loop form, so that a mis-copied field of the rebuilt struct changes bytes.  The global-pooling tail
(whose instances fetch three lines instead of five) gets pixel counts on both sides of a 16-pixel tile edge and of the wave count, in
both block widths, with traps for a lane that has no pixel of its own (it re-reads the last one): a leaked value changes an average
whose last pixel is non-zero in every channel, and a leaked 0 wins a maximum whose inputs are all negative."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from helpers import _scales, conv_graph, geom_params, conv_geom, pwdw_graph
from oracle import oracle
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_INT8, DT_INT32, Graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = [False, True]          # direct_dispatch


def run(g, x, direct, cfg=None, env=None):
    """every output and the launch list, pairs always fused"""
    old = {k: os.environ.get(k) for k in ["TAMD_FUSE_PWDW", "TAMD_PIN"] + list(env or {})}
    os.environ["TAMD_FUSE_PWDW"] = "2"
    if cfg:
        os.environ["TAMD_PIN"] = "pwdw_cfg=" + cfg.replace(",", "x")
    os.environ.update(env or {})
    try:
        gr = capi.Graph(tm2.write_tm2(g), direct_dispatch=direct)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    gr.set_input(x)
    outs = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    return outs, names


def check(g, x, prefix, cfg=None, env=None, launches=1, want=None):
    want = oracle.run_graph(g, x) if want is None else want
    assert len(np.unique(want[0])) >= 3
    for direct in PATHS:
        outs, names = run(g, x, direct, cfg, env)
        assert len(names) == launches and all(n.startswith(prefix) for n in names), names
        for got, ref in zip(outs, want):
            bad = np.count_nonzero(got.reshape(ref.shape) != ref)
            assert bad == 0, "%s direct=%s: %d / %d bytes differ" % (names, direct, bad, ref.size)
    return names


# ---- every field of the rebuilt struct ------------------------------------------------------------------------------------------

def test_stride1_two_outputs_per_lane():
    """MODE 1 needs TH * ceil(TW / 2) * 4 >= threads: the whole 14 x 14 map in one 256-thread block"""
    g, x = pwdw_graph(2101, 1, 64, 14, 14, 32, 1, 1)
    assert check(g, x, "pwdw_i8", "14,14,256") == ["pwdw_i8<s1,14x14,256>"]


def test_stride2():
    g, x = pwdw_graph(2102, 1, 64, 7, 7, 32, 2, 1)
    assert check(g, x, "pwdw_i8", "4,4,256") == ["pwdw_i8<s2,4x4,256>"]


def test_stride1_one_output_per_lane():
    g, x = pwdw_graph(2103, 1, 64, 5, 9, 32, 1, 1, act_pw=6)
    assert check(g, x, "pwdw_i8", "5,9,256") == ["pwdw_i8<s1,5x9,256>"]


def test_no_tail_fc_on_a_1x1_map():
    """MODE 4: the lean slice kernel without a tail, pinned by name among the GEMM family"""
    g, x = conv_graph(2104, 1, 64, 1, 1, 40, 1)
    names = check(g, x, "pw_small_i8", env={"TAMD_FORCE_GEMM": "pw_small"})
    assert names == ["pw_small_i8<1>"]


def test_first_conv_producer():
    """PROD 1: 3 channels gathered from the NCHW graph input (taps, in_C / in_H / in_W, the first conv's stride and pads)"""
    g, x = pwdw_graph(2105, 1, 3, 18, 14, 16, 1, 1, first=(3, 2, 1))
    x[:] = np.random.default_rng(5).integers(-127, 128, size=x.shape)
    assert check(g, x, "firstdw_i8", "5,7,256") == ["firstdw_i8<s1,5x7,256>"]


def test_two_slices_per_block():
    g, x = pwdw_graph(2106, 2, 64, 5, 9, 32, 1, 1)
    assert check(g, x, "pwdw_i8", "5,7,256,2") == ["pwdw_i8<s1,5x7,256,c32>"]


def test_chunked_k_1088():
    """17 steps of 64: four in registers, the panel re-read per tile"""
    g, x = pwdw_graph(2107, 1, 1088, 7, 7, 16, 1, 1)
    assert check(g, x, "pwdw_i8", "7,7,256") == ["pwdw_i8<s1,7x7,256>"]


def test_batch_3_division_branch():
    g, x = pwdw_graph(2108, 3, 64, 5, 9, 32, 2, 1, act_dw=6)
    assert check(g, x, "pwdw_i8", "2,3,256") == ["pwdw_i8<s2,2x3,256>"]


def test_ragged_cout_40_of_48():
    """c_limit: the last slice stores 8 of its 16 channels"""
    g, x = pwdw_graph(2109, 1, 64, 7, 7, 40, 1, 1)
    check(g, x, "pwdw_i8", "7,7,256")


def concat_view_graph(seed, n, cin, h, w, ca, cb):
    """two pointwise + depthwise pairs on one input, concatenated along the channels with one scale: both depthwise outputs are
    views of the concat buffer, the second at channel offset `ca` (c_off, ldc = ca + cb)"""
    rng = np.random.default_rng(seed)
    g = Graph(name="pwdw_concat_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    x = g.add_input("data", [n, cin, h, w], DT_INT8, [xs], [0])
    F, D = conv_geom(None, 1, 1, 0), conv_geom(None, 3, 1, 1)
    outs, os_ = [], None
    for tag, c in (("a", ca), ("b", cb)):
        ws = _scales(rng, c)
        ins = [x, g.add_const("w_pw_" + tag, rng.integers(-127, 128, size=(c, cin, 1, 1)).astype(np.int8), DT_INT8, ws, [0] * c),
               g.add_const("b_pw_" + tag, rng.integers(-2000, 2000, size=(c,)).astype(np.int32), DT_INT32, [1.0], [0])]
        ms = float(np.float32(xs * np.mean(ws) * 73.0 * np.sqrt(cin) * 73.0 / 60.0))
        mid = g.add_tensor("mid_" + tag, [n, c, h, w], DT_INT8, tm2.TT_VAR, None, [ms], [0])
        g.add_node("pw_" + tag, "Convolution", ins, [mid], input_channel=cin, output_channel=c, group=1, activation=0, **geom_params(F))
        dsc = _scales(rng, c)
        dins = [mid, g.add_const("w_dw_" + tag, rng.integers(-127, 128, size=(c, 1, 3, 3)).astype(np.int8), DT_INT8, dsc, [0] * c),
                g.add_const("b_dw_" + tag, rng.integers(-2000, 2000, size=(c,)).astype(np.int32), DT_INT32, [1.0], [0])]
        if os_ is None:
            os_ = float(np.float32(ms * np.mean(dsc) * 73.0 * 3.0 * 73.0 / 60.0))
        y = g.add_tensor("out_" + tag, [n, c, h, w], DT_INT8, tm2.TT_VAR, None, [os_], [0])
        g.add_node("dw_" + tag, "Convolution", dins, [y], input_channel=c, output_channel=c, group=c, activation=0, **geom_params(D))
        outs.append(y)
    cat = g.add_tensor("cat", [n, ca + cb, h, w], DT_INT8, tm2.TT_VAR, None, [os_], [0])
    g.output_nodes = [g.add_node("cat", "Concat", outs, [cat], axis=1)]
    return g, rng.integers(-127, 128, size=(n, cin, h, w)).astype(np.int8)


def test_channel_offset_into_a_concat_view():
    """c_off and ldc.  (A view needs a channel count that is a multiple of 16 -- plan_concat_views -- so the ragged width is the case
    above and the offset is this one: 48 channels behind 32, rows of 80.)"""
    g, x = concat_view_graph(2110, 1, 64, 7, 7, 32, 48)
    check(g, x, "pwdw_i8", "7,7,256", launches=2)


# ---- the global-pooling tail ------------------------------------------------------------------------------------------------------

POOL_MAPS = [(1, 1), (3, 5), (4, 4), (1, 17), (3, 11), (7, 7), (8, 8), (5, 13)]      # 1, 15, 16, 17, 33, 49, 64, 65 pixels


@functools.lru_cache(maxsize=None)
def avg_case(n, cin, h, w, c):
    """a seeded pair (no activation on the pointwise conv) whose pointwise output is non-zero in every channel of the last pixel of every image"""
    for seed in range(3000 + 97 * h + 7 * w + cin + c + n, 3400 + 97 * h + 7 * w + cin + c + n):
        g, x = pwdw_graph(seed, n, cin, h, w, c, act_pw=-1, tail="pool", pool_alg=1, mid_output=True)
        mid = oracle.run_graph(g, x)[0]
        if np.all(mid.reshape(n, c, h, w)[:, :, -1, -1] != 0):
            return pwdw_graph(seed, n, cin, h, w, c, act_pw=-1, tail="pool", pool_alg=1)
    raise AssertionError("no seed with a non-zero last pixel")


@functools.lru_cache(maxsize=None)
def max_case(n, cin, h, w, c):
    """no activation on the pointwise conv (activation -1), small weights and a bias far below zero: every pointwise output is negative"""
    g, x = pwdw_graph(3500 + 97 * h + 7 * w + cin + c + n, n, cin, h, w, c, tail="pool", pool_alg=0, act_pw=-1, mid_output=True)
    rng = np.random.default_rng(h * w + c)
    for t in g.tensors:
        if t.name == "w_pw":
            t.data = rng.integers(-20, 21, size=t.data.shape).astype(np.int8)
        if t.name == "b_pw":
            t.data = np.full(t.data.shape, -int(5700 * np.sqrt(cin)), np.int32)
    mid = oracle.run_graph(g, x)[0]
    assert mid.max() < 0
    g.output_nodes = g.output_nodes[1:]
    return g, x


@pytest.mark.parametrize("h,w", POOL_MAPS)
@pytest.mark.parametrize("alg", [0, 1], ids=["max", "avg"])
def test_pointwise_plus_global_pool(alg, h, w):
    for c in (16, 40):
        for cin in (64, 192):
            for n in (1, 3):
                g, x = (avg_case if alg else max_case)(n, cin, h, w, c)
                want = oracle.run_graph(g, x)
                if alg == 0:
                    assert want[0].max() < 0          # a leaked identity (0) would win
                for threads in (256, 512):
                    for direct in PATHS:
                        outs, names = run(g, x, direct, "1,1,%d" % threads)
                        assert names == ["pwpool_i8<%d>" % threads], names
                        assert np.array_equal(outs[0].reshape(want[0].shape), want[0]), (alg, h, w, c, cin, n, threads, direct)


# ---- the flagship ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direct", PATHS, ids=["hipgraph", "direct"])
def test_mobilenet_v1_int8_batch1_matches_the_reference_sha(direct):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_outputs_sha256.json")))["mobilenet_v1_int8_b1"]
    g = models.build("mobilenet_v1", "int8", 1)
    gr = capi.Graph(tm2.write_tm2(g), batch=1, direct_dispatch=direct)
    gr.set_input(models.synth_input(g, 1000, DT_INT8))
    outs = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    assert sum(n.startswith(("pwdw_i8", "pwpool_i8")) for n in names) >= 8, names
    assert [hashlib.sha256(np.ascontiguousarray(o).tobytes()).hexdigest() for o in outs] == [o["sha256"] for o in golden["outputs"]]
