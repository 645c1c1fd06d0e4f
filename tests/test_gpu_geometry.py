"""Anisotropic and asymmetric convolution / pooling geometry on the device, in all three precisions: stride, pad, dilation and kernel
that differ between height and width, pad_*0 != pad_*1 (the (0,1,0,1) stride-2 layers of TF-converted models), and the reference's SAME
pad codes.  The cases are tests/geometry_cases.py's; the CPU suite pins the oracle to the real reference on every one of them
(test_oracle_vs_reference.py, test_uint8_oracle.py, test_fp32_oracle.py) and shows that exchanging pad_*0 and pad_*1 changes the
expected bytes (test_geometry_cases_discriminate).  Here: device == oracle -- bytes for int8 and uint8, ATOL = 1e-4 absolute for fp32
(test_gpu_parity_fp32.py's bar) -- with the kernel every case ran asserted through profile(), for every member of the int8 GEMM
family, every depthwise form, both first-layer kernels, every fused launch (against the same graph unfused on the device as well)
and every pinned form of the uint8 planner."""
import os

import numpy as np
import pytest

from geometry_cases import ALL_CONV, F32_WINO, FUSED, POOLS, fused_graph, not_degenerate, seed_of
from helpers import conv_graph, pinned, pool_graph, u8_conv_graph, u8_conv_int_model, u8_pool_graph
from oracle import oracle
from tengine_amd import capi, tm2
from test_gpu_gemm_family import MEMBERS
from test_gpu_parity_fp32 import ATOL, conv_graph_f32, pool_graph_f32

pytestmark = pytest.mark.gpu

GROUP1 = sorted(k for k in ALL_CONV if k.split("/")[0] in ("gemm", "same") and ALL_CONV[k][5] == 1)      # inner group-1 convolutions
FIRST = sorted(k for k in ALL_CONV if k.startswith("first/"))
DW3X3 = sorted(k for k in ALL_CONV if k.startswith("dw3x3/")) + ["same/same_dw_s2_b1"]
DIRECT = sorted(k for k in ALL_CONV if k.startswith("direct/"))
BUILDERS = {"i8": conv_graph, "u8": u8_conv_graph, "f32": conv_graph_f32}
_cache = {}


def case(dtype, name):
    """(graph, tmfile bytes, input, the oracle's output) of a convolution case: computed once, shared, never modified"""
    if (dtype, name) not in _cache:
        n, cin, h, w, cout, group, act, geom = ALL_CONV.get(name) or F32_WINO[name]
        g, x = BUILDERS[dtype](seed_of(name), n, cin, h, w, cout, 1, group=group, act=act, geom=geom)
        want = oracle.run_graph(g, x)[0]
        assert dtype == "f32" or not_degenerate(want), name
        assert want.shape[2] != want.shape[3] or name.endswith("pw_one_padded_column"), (name, want.shape)
        _cache[(dtype, name)] = (g, tm2.write_tm2(g), x, want)
    return _cache[(dtype, name)]


def fused_case(name, n):
    if ("fused", name, n) not in _cache:
        g, x = fused_graph(name, n)
        want = oracle.run_graph(g, x)[0]
        assert not_degenerate(want), (name, n)
        _cache[("fused", name, n)] = (g, tm2.write_tm2(g), x, want)
    return _cache[("fused", name, n)]


def device(tmb, x, pins=None, env=None, **kw):
    """-> (outputs, launch list); pins: TAMD_PIN keys, env: other switches, both in force around the prerun only"""
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update({k: str(v) for k, v in (env or {}).items()})
    try:
        with pinned(**(pins or {})):
            gr = capi.Graph(tmb, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    gr.set_input(x)
    outs = [np.array(o) for o in gr.run()]
    names = [k["kernel"] for k in gr.profile(1)]
    gr.close()
    return outs, names


def exact(got, want, what):
    got = got.reshape(want.shape)
    bad = np.count_nonzero(got != want)
    assert bad == 0, "%s: %d / %d bytes differ from the oracle (max |d| %d)" % (what, bad, want.size, np.abs(got.astype(int) - want.astype(int)).max())


def close(got, want, what):
    d = float(np.abs(got.reshape(want.shape).astype(np.float64) - want.astype(np.float64)).max())
    print("fp32 %s: max |d| = %.3g (|ref| max %.3g)" % (what, d, float(np.abs(want).max())))
    assert d <= ATOL, "%s: max |d| %g" % (what, d)


# ---- int8: the GEMM family ------------------------------------------------------------------------------------------------------
GEMM_KERNELS = ("conv_igemm", "gemm_direct", "pw_stream", "pw_rows", "pw_small", "conv_pgemm")
# Members whose own acceptance rule admits none of these shapes: the pointwise-only kernels (no case is an unpadded 1x1 / stride 1:
# pw_stride_w strides, pw_one_padded_column has a trailing pad -- ConvArgs holds the leading pads only, so conv_is_pointwise also asks
# OH == H and OW == W), conv_igemm2 (fewer than 64 blocks), and the 64-pixel x 128-cout conv_pgemm tile (more than 64 outputs: only
# k64_two_groups, a 3x3, which belongs to the dedicated 3x3 kernels -- and their 64x128 form is in experiment builds only).  Forced,
# they must decline every shape.
POINTWISE_ONLY = ("gemm_direct", "pw_stream", "pw_rows", "pw_small")
DECLINES_ALL = set(POINTWISE_ONLY) | {"conv_igemm2", "conv_pgemm_i8<64x128"}
# TAMD_FORCE_GEMM=igemm<k> -> the kernel name of tile configuration k (conv_igemm.hip: conv_igemm_kernel_name)
IGEMM_NAMES = ["conv_igemm_i8<128x128x64>", "conv_igemm_i8<128x32x64>", "conv_igemm_i8<64x64x64>", "conv_igemm_i8<32x128x64>", "conv_igemm_i8<128x64x64>",
               "conv_igemm_i8<128x128x256>", "conv_igemm_i8<128x64x256>", "conv_igemm_i8<64x64x256>", "conv_igemm_i8<64x64x128>", "conv_igemm_i8<128x64x128>",
               "conv_igemm_i8<128x128x64,ring>", "conv_igemm_i8<128x64x64,ring>", "conv_igemm_i8<256x64x64,ring>", "conv_igemm_i8<64x128x64,ring>",
               "conv_igemm_i8<64x64x64,ring>", "conv_igemm_i8<256x128x64,ring>"]


@pytest.mark.parametrize("member", [None] + MEMBERS, ids=["default"] + MEMBERS)
def test_int8_gemm_family(member):
    used = []
    for name in GROUP1:
        g, tmb, x, want = case("i8", name)
        outs, names = device(tmb, x, env={"TAMD_FORCE_GEMM": member} if member else None)
        print(member, name, names)
        assert len(names) == 1 and names[0].startswith(GEMM_KERNELS), (name, names)
        exact(outs[0], want, "%s %s (%s)" % (member, name, names[0]))
        if member and names[0].startswith(IGEMM_NAMES[int(member[5:])] if member.startswith("igemm") else member):
            used.append(name)
    if member in DECLINES_ALL:
        assert not used, (member, used)
    elif member:
        assert used, "%s ran on none of %s" % (member, GROUP1)


def test_pointwise_with_a_trailing_pad_is_not_run_as_a_pointwise_gemm():
    """pad_w1 = 1 on a 1x1 layer, stride 1 (the output map is one column wider than the input) and stride 2 (its last column starts at
    x = W): that column holds the requantised bias.  The pointwise-only members (output pixel m reads input pixel m) and conv_pgemm's
    rows form (pixel (oy*SH, ox*SW), unchecked) must decline both, forced or not."""
    for name in ("gemm/pw_one_padded_column", "gemm/pw_tf_same_s2"):
        g, tmb, x, want = case("i8", name)
        bias_only = oracle.run_graph(g, np.zeros_like(x))[0]
        assert np.array_equal(want[..., -1], bias_only[..., -1]) and len(np.unique(want[..., -1])) > 4      # the column no input reaches
        for member in POINTWISE_ONLY + ("conv_pgemm_i8<64x64", "conv_pgemm_i8<128x64"):
            outs, names = device(tmb, x, env={"TAMD_FORCE_GEMM": member})
            assert not names[0].startswith(POINTWISE_ONLY) and "rows" not in names[0], (name, member, names)
            exact(outs[0], want, "%s forced %s (%s)" % (name, member, names[0]))


# ---- int8: depthwise 3x3, generic direct, first layer ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", [None, 11, 12, 14, 21, 22])
@pytest.mark.parametrize("name", DW3X3)
def test_int8_depthwise_3x3(name, form):
    """the dwconv3x3 launch in every form dwconv.hip's dw_form pin accepts; dw_tf_same_s2_b1 and same_dw_s2_b1 carry the REF formula at
    batch 1 (pads not pairwise equal: conv_mode), dw_ph_ne_pw_b1 the HCL formula with PH != PW, dw_ragged_b3 the batched one"""
    g, tmb, x, want = case("i8", name)
    outs, names = device(tmb, x, pins={"dw_form": form} if form else None)
    s = ALL_CONV[name][7]["sh"]
    if form:
        nf, th = divmod(form, 10)
        assert names == ["dwconv3x3_i8<%d,%d%s>" % (s, nf, ",r%d" % th if th > 1 else "")], names
    else:
        assert len(names) == 1 and names[0].startswith("dwconv3x3_i8<%d," % s), names
    exact(outs[0], want, "%s %s" % (name, names[0]))


@pytest.mark.parametrize("name", DIRECT)
def test_int8_generic_direct(name):
    g, tmb, x, want = case("i8", name)
    outs, names = device(tmb, x)
    assert names == ["conv_direct_i8"], names
    exact(outs[0], want, name)


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "gather"])
@pytest.mark.parametrize("name", FIRST)
def test_int8_first_layer(name, rows):
    """conv_first_i8 with its row-granular loads and (first_rows=0) its generic gather; an input of more than 4 channels is not read in
    NCHW by the convolution: first_8ch_3x2 is a GEMM-family launch like any inner layer"""
    g, tmb, x, want = case("i8", name)
    outs, names = device(tmb, x, pins=None if rows else {"first_rows": 0})
    if ALL_CONV[name][1] > 4:
        assert len(names) == 1 and names[0].startswith(GEMM_KERNELS), names
    else:
        assert names == ["conv_first_i8"], names
    exact(outs[0], want, name)


# ---- int8: fused launches --------------------------------------------------------------------------------------------------------
def fused_and_unfused(name, n, on, off, is_fused, launches_off):
    """runs the graph with the switches `on` and `off` ((pins, env) each): one fused launch / `launches_off` launches, both the oracle's
    bytes, and the same bytes as each other"""
    g, tmb, x, want = fused_case(name, n)
    outs, names = device(tmb, x, pins=on[0], env=on[1])
    print(name, n, names)
    assert len(names) == 1 and is_fused(names[0]), names
    exact(outs[0], want, "%s b%d %s" % (name, n, names[0]))
    outs0, names0 = device(tmb, x, pins=off[0], env=off[1])
    assert len(names0) == launches_off and not any(is_fused(k) for k in names0), names0
    exact(outs0[0], want, "%s b%d unfused" % (name, n))
    assert np.array_equal(outs[0], outs0[0])
    return names[0]


PAIRS = [(name, n) for name in ("firstdw_tf_stem", "firstdw_tf_stem_same", "firstdw_3x4_dilh2", "pwdw_tf_s2", "pwdw_s1_p2012") for n in FUSED[name]]


@pytest.mark.parametrize("name,n", PAIRS, ids=["%s-b%d" % c for c in PAIRS])
def test_int8_conv_plus_depthwise_pairs(name, n):
    """first conv -> dw and pw -> dw as one launch: the default plan at batch 1 (HCL or, with pads not pairwise equal, REF depthwise
    formula), TAMD_FUSE_PWDW=2 at batch > 1 (REF formula)"""
    kind = "firstdw" if name.startswith("firstdw") else "pwdw"
    got = fused_and_unfused(name, n, (None, {"TAMD_FUSE_PWDW": 2} if n > 1 else None), (None, {"TAMD_FUSE_PWDW": 0}),
                            lambda k: k.split("_i8")[0] in ("pwdw", "firstdw"), 2)
    assert got.startswith(kind + "_i8<s%d," % (2 if name in ("firstdw_3x4_dilh2", "pwdw_tf_s2") else 1)), got


def test_int8_depthwise_plus_pointwise():
    fused_and_unfused("dwpw_p1001", 2, (None, {"TAMD_FUSE_DWPW": 2}), (None, {"TAMD_FUSE_DWPW": 0}), lambda k: k == "dwpw_i8", 2)


CHAINS = [(name, n, cfg) for name in ("chain_pw", "chain_first") for n in FUSED[name] for cfg in (None, "2x2x256")]


@pytest.mark.parametrize("name,n,cfg", CHAINS, ids=["%s-b%d-%s" % (a, b, c or "auto") for a, b, c in CHAINS])
def test_int8_chain4(name, n, cfg):
    """dw1 pads (0,1,1,0), dw2 stride 2 pads (0,1,0,1), behind a pointwise conv and behind a 3x3 / s2 / (0,1,0,1) first conv"""
    pin = dict(chain4=2, **({"chain4_cfg": cfg} if cfg else {}))
    got = fused_and_unfused(name, n, (pin, {"TAMD_FUSE_PWDW": 2}), ({"chain4": 0}, {"TAMD_FUSE_PWDW": 2}),
                            lambda k: k.split("_i8")[0] in ("chain4", "firstchain4"), 2)
    assert got.startswith(("firstchain4" if name == "chain_first" else "chain4") + "_i8<s2,"), got
    if cfg:
        assert got.endswith(",2x2,256>"), got


def test_int8_chain4_under_direct_dispatch():
    from test_gpu_chain4 import is_chain, run
    g, tmb, x, want = fused_case("chain_first", 1)
    outs, names, packets = run(g, x, "chain4=2", direct=True, fuse_pwdw=2)
    assert len(names) == 1 and is_chain(names[0]) and names[0].startswith("firstchain4"), names
    # exactly one packet is the coherent chain instance, no pair kernel beside it: no fall-back to hipGraph replay
    assert sum("chain4_i8_coh_kernel" in p for p in packets) == 1 and not any("pwdw_i8" in p for p in packets), packets
    exact(outs[0], want, "chain_first direct dispatch")


def test_int8_block_with_unequal_pads_is_not_the_block_kernel():
    """the 3x3 with pads (2,0,1,1) keeps the map size but is not block_i8's geometry: bytes == oracle either way; block_i8 only if exact"""
    g, tmb, x, want = fused_case("block_p2011", 2)
    outs, names = device(tmb, x, env={"TAMD_FUSE_BLOCK": 1})
    outs0, names0 = device(tmb, x, env={"TAMD_FUSE_BLOCK": 0})
    print(names, names0)
    exact(outs[0], want, "block switch on %s" % names)
    exact(outs0[0], want, "block switch off")
    assert "block_i8" not in names0
    assert "block_i8" in names or names == names0, (names, names0)


def test_int8_stem_and_relu_with_a_3x2_pool():
    """pool 3x2 / stride (2,1) / pads (1,0) behind the first conv and behind a ReLU, each with its fusion on and off"""
    g, tmb, x, want = fused_case("stem_pool_3x2", 1)
    for on in (1, 0):
        outs, names = device(tmb, x, pins={"first_pool": on})
        assert names == ["conv_first_i8", "pool_i8"], names           # (conv_first_pool_i8 takes MAX 3x3 / 2 / pad 0 only)
        exact(outs[0], want, "stem, first_pool=%d" % on)
    g, tmb, x, want = fused_case("relu_pool_3x2", 2)
    outs, names = device(tmb, x)
    assert names == ["relu_pool_i8"], names
    exact(outs[0], want, "relu_pool_i8")
    outs0, names0 = device(tmb, x, pins={"relu_pool": 0})
    assert names0 == ["relu_i8", "pool_i8"], names0
    exact(outs0[0], want, "relu + pool")


# ---- pools, all three precisions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(POOLS))
def test_pools(name):
    n, c, h, w, alg, caffe, geom = POOLS[name]
    for dtype, build, kernel in (("i8", lambda: pool_graph(seed_of(name), n, c, h, w, alg, 0, 0, caffe=caffe, geom=geom), "pool_i8"),
                                 ("u8", lambda: u8_pool_graph(seed_of(name), n, c, h, w, alg, 0, 0, caffe=caffe, geom=geom), "pool_u8"),
                                 ("f32", lambda: pool_graph_f32(seed_of(name), n, c, h, w, alg, caffe, geom), "pool_f32")):
        g, x = build()
        want = oracle.run_graph(g, x)[0]
        assert want.shape[2] != want.shape[3] and len(np.unique(want)) >= 16
        outs, names = device(tm2.write_tm2(g), x)
        assert names == [kernel], names
        if dtype == "f32":
            close(outs[0], want, name)
        else:
            exact(outs[0], want, "%s %s" % (dtype, name))


# ---- uint8 -----------------------------------------------------------------------------------------------------------------------
# the pinned forms of the uint8 planner, with the values test_gpu_u8_patch.py / test_gpu_u8_lanes.py / test_gpu_parity_uint8.py use;
# a pin takes its kernel wherever that kernel's own rule admits the shape, every other shape keeps its form
U8_PINS = {"default": {}, "patch": {"u8_patch": 1}, "lanes": {"u8_patch": 1, "u8_patch_cfg": 4}, "no_patch": {"u8_patch": 0}, "no_lanes": {"u8_lanes": 0},
           "pw": {"u8_patch": 0, "u8_pw": 1}, "no_pw": {"u8_patch": 0, "u8_pw": 0}, "c3": {"u8_patch": 0, "u8_c3": 1}, "no_c3": {"u8_patch": 0, "u8_c3": 0},
           "rgb3x3": {"u8_rgb3x3": 1}}
U8_KERNELS = ("conv_u8_", "dequant_u8_f32")


@pytest.mark.parametrize("form", sorted(U8_PINS))
def test_uint8_group1_and_first_layer(form):
    """the GEMM, first-layer and SAME tables (zero points 112..143: a padded tap is visible) under every pinned form: bytes"""
    ran = {}
    for name in GROUP1 + FIRST:
        g, tmb, x, want = case("u8", name)
        outs, names = device(tmb, x, pins=U8_PINS[form])
        print(form, name, names)
        assert names and all(k.startswith(U8_KERNELS) for k in names) and not any("conv_u8_direct" in k for k in names), (name, names)
        exact(outs[0], want, "%s %s %s" % (form, name, names))
        ran[name] = names[-1]
    if form == "patch":
        assert sum("conv_u8_patch" in k for k in ran.values()) >= 1, ran
    if form == "lanes":
        assert sum("conv_u8_lanes" in k for k in ran.values()) >= 1, ran
    if form in ("no_patch", "no_pw", "no_c3"):
        assert not any("conv_u8_patch" in k or "conv_u8_lanes" in k for k in ran.values()), ran
    if form == "no_lanes":
        assert not any("conv_u8_lanes" in k for k in ran.values()), ran
    if form == "pw":          # a strided 1x1 and a 1x1 with a trailing pad are not the pointwise kernel's (H == OH and W == OW)
        assert not any("conv_u8_pw" in k for k in ran.values()), ran
    if form == "c3":          # 3x3 without dilation on whole 16-channel steps, any stride pair: stride_h_only among them
        assert "conv_u8_c3" in ran["gemm/stride_h_only"], ran
    if form == "rgb3x3":      # 3x3 without dilation on <= 4 channels
        assert "conv_u8_rgb3x3" in ran["first/first_3x3_s21"], ran


@pytest.mark.parametrize("name", DW3X3 + DIRECT)
def test_uint8_depthwise_and_grouped(name):
    g, tmb, x, want = case("u8", name)
    outs, names = device(tmb, x)
    assert names == ["conv_u8_direct"], names
    exact(outs[0], want, name)


def test_uint8_integer_path():
    """one pass of the group-1 tables through the opt-in integer path, at test_gpu_u8_int.py's bar: byte-exact against the
    operation-for-operation model of the integer formula, within one quantisation step of the reference's bytes with a mismatch
    fraction below 2e-3; a shape the integer kernels do not take keeps its byte-exact form"""
    took = 0
    for name in GROUP1 + FIRST:
        if name.startswith("same/"):
            continue                      # (the model takes explicit pads)
        g, tmb, x, want = case("u8", name)
        outs, names = device(tmb, x, u8_integer=True)
        got = outs[0].reshape(want.shape)
        if any(k.startswith("conv_u8i") for k in names):
            model = u8_conv_int_model(g, x)
            bad = np.count_nonzero(got != model)
            assert bad == 0, "%s %s: %d / %d bytes differ from the integer model" % (name, names, bad, model.size)
            d = np.abs(model.astype(int) - want.astype(int))
            print("integer path %s %s: max |d| %d, %d of %d differ from the reference" % (name, names, d.max(), np.count_nonzero(d), d.size))
            assert d.max() <= 1 and np.count_nonzero(d) / d.size < 2e-3, name
            took += 1
        else:
            exact(got, want, "%s (exact form %s)" % (name, names))
    assert took >= 6, took


# ---- fp32 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUP1 + FIRST)
def test_fp32_gemm(name):
    g, tmb, x, want = case("f32", name)
    outs, names = device(tmb, x, env={"TAMD_F32_WINOGRAD": 0})
    assert len(names) == 1 and names[0].startswith("conv_f32_mfma"), names
    close(outs[0], want, "%s %s" % (name, names[0]))


@pytest.mark.parametrize("name", DW3X3 + DIRECT)
def test_fp32_depthwise_and_grouped(name):
    g, tmb, x, want = case("f32", name)
    outs, names = device(tmb, x)
    assert names == ["conv_f32_direct"], names
    close(outs[0], want, name)


@pytest.mark.parametrize("name", sorted(F32_WINO))
def test_fp32_winograd_forced(name):
    g, tmb, x, want = case("f32", name)
    outs, names = device(tmb, x, env={"TAMD_F32_WINOGRAD": 1})
    assert names == ["wino_in_f32", "wino_gemm_f32<F(2,3)>", "wino_out_f32"], names
    close(outs[0], want, "%s F(2,3)" % name)
    direct, names0 = device(tmb, x, env={"TAMD_F32_WINOGRAD": 0})
    assert len(names0) == 1 and names0[0].startswith("conv_f32_mfma"), names0
    close(direct[0], want, "%s direct" % name)
    assert np.abs(direct[0] - outs[0]).max() <= 2e-4 * max(1.0, np.abs(want).max())
