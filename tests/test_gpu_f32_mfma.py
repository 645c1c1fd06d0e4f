"""conv_f32_mfma.hip in all five tile configurations and both chain forms, each configuration pinned with TAMD_PIN=f32_cfg=<c> and the
kernel name asserted through profile(1).

fp32 form (tail_split = 0: every pixel is one fused chain in ascending k): group-1 convolutions and FullyConnected of fp32 graphs against
oracle.run_graph at test_gpu_parity_fp32.py's ATOL (1e-4 absolute), finite normal(0,1) inputs and He-scaled weights.  The tables aim at
the kernel's own branches, at the smallest shapes that reach them -- BM x BN being the configuration's tile:
  K ladder        nstage 1..9: every `rem` branch of the s_waitcnt vmcnt ladder for STAGES 4, 5 and 6, the p < nstage prologue guard, a
                  ragged last stage
  pixel edges     OH*OW around the 16 / 32 / 64 pixel tiles, N = 3 (a pixel tile never straddles images)
  channel tiles   CT = 1 .. 17 with a ragged last tile: the plain block order below 8 channel tiles, the XCD swizzle with its early return
                  from 8 on
  zero-page taps  stride, dilation, a kernel larger than the map, 1x7 and 7x1
  Concat slice    out_c0 != 0 and out_img > cout*OH*OW; the whole Concat is compared
  FullyConnected  as_fc: the flattened input is the K axis, N pixel tiles of one pixel
Every shape that a table derives from one BM (cout = BM + 3 ...) runs in ALL five configurations, and the five outputs must be
bit-identical: the file header of conv_f32_mfma.hip states that every configuration feeds one accumulator in ascending k and that a
padded k row contributes fma(0, x, s) = s.

uint8 LDS-DMA form (tail_split = 1, the byte-exact fallback for rup(K,64) > 29184): helpers.u8_conv_graph with K past that limit, so the
planner takes conv_u8_dma by itself; bytes == oracle.run_graph in every configuration.  The shapes reach what the TAIL body (the
reference's four interleaved chains for the last OH*OW % 8 pixels) had never run on the device: K % 4 = 1, 2, 3 (the remainder loop's own
index into the packed weights), rows outside the 8- and 4-row blocks (co >= m_blocked), TM > 1 and TN > 1, a tail-only image, several
images and several channel tiles.  What bytes can show: a wrong weight or tap index, a skipped or doubled k row, a missing bias or a row
written to the wrong place moves a sum by far more than a quantisation step and fails with certainty; a wrong ORDER of the same addends
moves a sum by an ulp and shows only where that sum sits on a rounding boundary (the campaign of tools/fuzz_device.py, which now pins
f32_cfg too, is the statistical check of that).

The last test is a census: every kernel name ran in both forms, and the TAIL cases covered K % 4 in {0,1,2,3} on both sides of m_blocked."""
import functools

import numpy as np
import pytest

from helpers import u8_conv_graph
from oracle import oracle
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, Graph
from test_gpu_parity_fp32 import ATOL, close, conv_graph_f32

pytestmark = pytest.mark.gpu

# conv_f32_mfma.hip: F32_CFGS -- (BM output channels, BN pixels, kernel name) of f32_cfg = 0..4
F32_CFGS = [(16, 64, "conv_f32_mfma_16x64"), (32, 32, "conv_f32_mfma_32x32"), (64, 64, "conv_f32_mfma_64x64"),
            (32, 64, "conv_f32_mfma_32x64"), (64, 16, "conv_f32_mfma_64x16")]
CFGS = range(len(F32_CFGS))
BMS = sorted({c[0] for c in F32_CFGS})          # the distinct BM: a table's "BM + 3" is one shape per value, run in every configuration

RAN = {"fp32": set(), "dma": set()}             # form -> kernel names that profile(1) showed
TAILS = set()                                   # (K % 4, "blocked" / "single"): what the TAIL body's cases covered, by their shapes


def device(tmb, x, cfg, monkeypatch):
    """-> (outputs, launch list) with configuration `cfg` pinned and the direct form of every 3x3"""
    monkeypatch.setenv("TAMD_PIN", "f32_cfg=%d" % cfg)
    monkeypatch.setenv("TAMD_F32_WINOGRAD", "0")
    gr = capi.Graph(tmb)
    gr.set_input(x)
    outs = gr.run()
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    return outs, names


def five_ways(g, x, what, monkeypatch, launches=lambda name: [name]):
    """the graph in all five configurations: the launch list is `launches(kernel name)`, every output within ATOL of the oracle, and the
    five results bit-identical"""
    tmb = tm2.write_tm2(g)
    wants = oracle.run_graph(g, x)
    assert all(np.isfinite(w).all() and np.abs(w).max() > 1e-3 for w in wants), what
    first = None
    for c in CFGS:
        name = F32_CFGS[c][2]
        outs, names = device(tmb, x, c, monkeypatch)
        assert names == launches(name), (what, c, names)
        RAN["fp32"].add(name)
        assert len(outs) == len(wants)
        outs = [o.reshape(w.shape) for o, w in zip(outs, wants)]
        for o, w in zip(outs, wants):
            assert o.dtype == np.float32
            assert close(o, w, "%s %s" % (name, what)), "%s in %s: max |d| %g" % (what, name, np.abs(o - w).max())
        if first is None:
            first = outs
        for o, f in zip(outs, first):
            assert np.array_equal(o, f), "%s: %s and %s differ in %d of %d floats (max |d| %g)" % (
                what, name, F32_CFGS[0][2], np.count_nonzero(o != f), f.size, np.abs(o - f).max())


# ---- K ladder: 1x1, N = 2, 5x7 map, cout = BM + 3 -------------------------------------------------------------------------------------
K_LADDER = [1, 5, 31, 32, 33, 64, 95, 96, 128, 160, 161, 192, 224, 257]


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("cin", K_LADDER)
def test_k_ladder(cin, bm, monkeypatch):
    g, x = conv_graph_f32(7000 + cin + bm, 2, cin, 5, 7, bm + 3, 1, act=-1)
    five_ways(g, x, "k ladder cin %d cout %d" % (cin, bm + 3), monkeypatch)


# ---- pixel edges: cin 24, 3x3 pad 1, cout = BM, N = 3 ---------------------------------------------------------------------------------
PIXEL_MAPS = [(1, 1), (3, 5), (4, 4), (1, 17), (7, 9), (8, 8), (5, 13), (3, 43)]          # OH*OW = 1, 15, 16, 17, 63, 64, 65, 129


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("hw", PIXEL_MAPS, ids=["%dx%d" % m for m in PIXEL_MAPS])
def test_pixel_edges(hw, bm, monkeypatch):
    h, w = hw
    g, x = conv_graph_f32(7100 + h * w + bm, 3, 24, h, w, bm, 3, 1, 1, act=0)
    five_ways(g, x, "pixel edges %dx%d cout %d" % (h, w, bm), monkeypatch)


# ---- channel tiles and the XCD swizzle: cin 16, 1x1, 9x9 map, N = 2, cout = CT*BM - 5 -------------------------------------------------
CHANNEL_TILES = [1, 2, 7, 8, 9, 17]


@pytest.mark.parametrize("bm", BMS)
@pytest.mark.parametrize("ct", CHANNEL_TILES)
def test_channel_tiles_and_xcd_swizzle(ct, bm, monkeypatch):
    cout = ct * bm - 5
    g, x = conv_graph_f32(7200 + cout, 2, 16, 9, 9, cout, 1, act=-1)
    five_ways(g, x, "channel tiles CT %d of %d, cout %d" % (ct, bm, cout), monkeypatch)


# ---- zero-page taps: N = 2, cin 7, cout 13 ---------------------------------------------------------------------------------------------
ZERO_PAGE = {
    "3x3_stride2_pad1": (9, 11, dict(kh=3, kw=3, sh=2, sw=2, ph0=1, ph1=1, pw0=1, pw1=1)),
    "3x3_dilation2_pad2": (9, 11, dict(kh=3, kw=3, dh=2, dw=2, ph0=2, ph1=2, pw0=2, pw1=2)),
    "5x5_pad2_on_4x4": (4, 4, dict(kh=5, kw=5, ph0=2, ph1=2, pw0=2, pw1=2)),
    "1x7_pad3": (5, 9, dict(kh=1, kw=7, pw0=3, pw1=3)),
    "7x1_pad3": (9, 5, dict(kh=7, kw=1, ph0=3, ph1=3)),
}


@pytest.mark.parametrize("name", sorted(ZERO_PAGE))
def test_zero_page_taps(name, monkeypatch):
    h, w, geom = ZERO_PAGE[name]
    g, x = conv_graph_f32(7300 + len(name), 2, 7, h, w, 13, 1, act=-1, geom=geom)
    five_ways(g, x, "zero page %s" % name, monkeypatch)


# ---- into a Concat slice ---------------------------------------------------------------------------------------------------------------
def concat_graph_f32(seed, n, cin, h, w, couts):
    """data -> one 3x3 pad-1 convolution per entry of `couts`, each written in place into its channel slice -> Concat -> leaky ReLU"""
    rng = np.random.default_rng(seed)
    g = Graph(name="conv_concat_f32_case")
    x = g.add_input("data", [n, cin, h, w], DT_FP32, None, None)
    parts = []
    for i, cout in enumerate(couts):
        wt = g.add_const("w%d" % i, rng.normal(0, np.sqrt(2.0 / (cin * 9)), size=(cout, cin, 3, 3)).astype(np.float32), DT_FP32, None, None)
        b = g.add_const("b%d" % i, rng.uniform(-0.1, 0.1, size=(cout,)).astype(np.float32), DT_FP32, None, None)
        y = g.add_tensor("conv%d" % i, [n, cout, h, w], DT_FP32, tm2.TT_VAR, None, None, None)
        g.add_node("conv%d" % i, "Convolution", [x, wt, b], [y], kernel_h=3, kernel_w=3, stride_h=1, stride_w=1, dilation_h=1, dilation_w=1,
                   input_channel=cin, output_channel=cout, group=1, activation=-1, pad_h0=1, pad_w0=1, pad_h1=1, pad_w1=1)
        parts.append(y)
    cat = g.add_tensor("cat", [n, sum(couts), h, w], DT_FP32, tm2.TT_VAR, None, None, None)
    g.add_node("cat", "Concat", parts, [cat], axis=1)
    out = g.add_tensor("out", [n, sum(couts), h, w], DT_FP32, tm2.TT_VAR, None, None, None)
    g.output_nodes = [g.add_node("leaky", "ReLU", [cat], [out], negative_slope=0.1)]
    return g, rng.normal(0, 1, size=(n, cin, h, w)).astype(np.float32)


@pytest.mark.parametrize("bm", BMS)
def test_into_a_concat_slice(bm, monkeypatch):
    """the second convolution writes at out_c0 = 5 of an image of 5 + BM + 1 channels; both write in place (no concat_f32 launch), and a
    write outside either slice shows in the other's channels"""
    g, x = concat_graph_f32(7400 + bm, 2, 6, 5, 7, (5, bm + 1))
    five_ways(g, x, "concat slice couts 5 + %d" % (bm + 1), monkeypatch, launches=lambda name: [name, name, "relu_f32"])


# ---- FullyConnected ----------------------------------------------------------------------------------------------------------------------
def fc_graph_f32(seed, n, hidden_dims, nout, bias):
    rng = np.random.default_rng(seed)
    g = Graph(name="fc_f32_case")
    hidden = int(np.prod(hidden_dims))
    x = g.add_input("data", [n] + list(hidden_dims), DT_FP32, None, None)
    ins = [x, g.add_const("w", rng.normal(0, np.sqrt(2.0 / hidden), size=(nout, hidden)).astype(np.float32), DT_FP32, None, None)]
    if bias:
        ins.append(g.add_const("b", rng.uniform(-0.1, 0.1, size=(nout,)).astype(np.float32), DT_FP32, None, None))
    y = g.add_tensor("out", [n, nout], DT_FP32, tm2.TT_VAR, None, None, None)
    g.output_nodes = [g.add_node("fc", "FullyConnected", ins, [y], num_output=nout)]
    return g, rng.normal(0, 1, size=[n] + list(hidden_dims)).astype(np.float32)


FC_INPUTS = [(40,), (8, 3, 3), (257,)]
FC_NOUT = [1, 10] + [bm + 3 for bm in BMS] + [1000]


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("nout", FC_NOUT)
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("dims", FC_INPUTS, ids=["x".join(map(str, d)) for d in FC_INPUTS])
def test_fully_connected(dims, n, nout, bias, monkeypatch):
    g, x = fc_graph_f32(7500 + int(np.prod(dims)) + 7 * n + nout, n, dims, nout, bias)
    five_ways(g, x, "fc [%d,%s] -> %d %s" % (n, ",".join(map(str, dims)), nout, "bias" if bias else "no bias"), monkeypatch)


# ---- the byte-exact uint8 LDS-DMA form ---------------------------------------------------------------------------------------------------
DMA = [
    # n, cin, h, w, cout, k, s, p, group, act, bias, dil
    (2, 3243, 3, 5, 70, 3, 1, 1, 1, 0, True, 1),        # K % 4 = 3, 8 main + 7 tail pixels, two row singles (68, 69), 2 images
    (1, 3245, 2, 2, 13, 3, 1, 1, 1, -1, True, 1),       # K % 4 = 1, tail only (N8 == 0), 8-block + 4-block + one single
    (2, 3246, 4, 4, 23, 3, 1, 1, 1, 0, False, 1),       # K % 4 = 2, no tail block at all (16 pixels), no bias
    (1, 3244, 3, 3, 37, 3, 1, 1, 1, -1, False, 1),      # K % 4 = 0, one tail pixel, one single row
    (3, 3243, 1, 7, 9, 3, 1, 1, 1, 0, True, 1),         # 7 pixels, tail only, 3 images
    (2, 3245, 5, 5, 132, 3, 1, 1, 1, -1, True, 1),      # several channel tiles in every configuration, 24 + 1 pixels
    (1, 29187, 3, 5, 13, 1, 1, 0, 1, 0, True, 1),       # 1x1: the largest tap offsets the table holds here
    # the K % 4 = 2 row above has no tail pixel, so the TAIL body's remainder loop would never see two rows: 8 main + 1 tail pixel,
    # 8-block + 4-block + three singles (68 distinct bytes in the oracle's output, none at 0 / 255)
    (1, 3246, 1, 9, 15, 3, 1, 1, 1, -1, True, 1),
]


@functools.lru_cache(maxsize=None)
def dma_case(case):
    n, cin, h, w, cout, k, s, p, group, act, bias, dil = case
    g, x = u8_conv_graph(2000 + cin + cout + h, n, cin, h, w, cout, k, s, p, group, act, bias, dil)      # test_ragged_uint8_conv's seed rule
    want = oracle.run_graph(g, x)[0]
    want.setflags(write=False)
    return tm2.write_tm2(g), x, want


def check_dma(case, cfg, monkeypatch):
    n, cin, h, w, cout, k = case[:6]
    K = cin * k * k
    assert (K + 63) // 64 * 64 > 29184                 # graph_u8.hip u8_dma_wanted: the tap table no longer fits in LDS
    tmb, x, want = dma_case(case)
    # what keeps the case honest: the bytes are spread, and few of them sit at the clamps
    assert len(np.unique(want)) >= 16 and np.mean((want == 0) | (want == 255)) <= 0.5, case
    outs, names = device(tmb, x, cfg, monkeypatch)
    name = F32_CFGS[cfg][2]
    assert names == ["dequant_u8_f32", name], (case, cfg, names)
    got = outs[0].reshape(want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s in %s: %d of %d bytes differ from the oracle (max |d| %d), first at (n, c, y, x) = %s" % (
        case, name, len(bad), want.size, np.abs(got.astype(int) - want.astype(int)).max(), bad[0].tolist())
    RAN["dma"].add(name)
    if want.shape[2] * want.shape[3] % 8:              # the case has tail pixels: the TAIL body ran, on these rows
        m_blocked = cout // 8 * 8 + (cout % 8) // 4 * 4
        if m_blocked:
            TAILS.add((K % 4, "blocked"))
        if cout > m_blocked:
            TAILS.add((K % 4, "single"))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("case", DMA, ids=[str(c) for c in DMA])
def test_uint8_dma_form_is_byte_exact(case, cfg, monkeypatch):
    check_dma(case, cfg, monkeypatch)


# ---- census ------------------------------------------------------------------------------------------------------------------------------
def test_census_every_configuration_ran_in_both_forms(monkeypatch):
    """every kernel name was the pinned launch of an fp32 graph and of a uint8 DMA graph, and the TAIL body's cases covered K % 4 in
    {0, 1, 2, 3} on both sides of m_blocked (cases that were deselected in this run are run here)"""
    names = {c[2] for c in F32_CFGS}
    if RAN["fp32"] != names:
        test_k_ladder(33, 16, monkeypatch)
    for case in DMA:
        for cfg in CFGS:
            if RAN["dma"] != names or len(TAILS) < 8:
                check_dma(case, cfg, monkeypatch)
    print("fp32 form:", sorted(RAN["fp32"]), "\nuint8 DMA form:", sorted(RAN["dma"]), "\nTAIL cases (K % 4, rows):", sorted(TAILS))
    assert RAN["fp32"] == names and RAN["dma"] == names, RAN
    assert TAILS == {(r, side) for r in range(4) for side in ("blocked", "single")}, sorted(TAILS)
