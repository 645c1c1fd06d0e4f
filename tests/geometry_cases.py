"""Anisotropic / asymmetric convolution and pooling geometry: the case tables shared by the CPU pins (oracle == the real reference:
test_oracle_vs_reference.py, test_uint8_oracle.py, test_fp32_oracle.py) and the device tests (test_gpu_geometry.py).

Notation of a convolution case: (n, cin, h, w, cout, group, act, geom), geom = G((kh, kw), (sh, sw), (ph0, ph1, pw0, pw1)[, (dh, dw)]).
Every case has H != W and OH != OW (pw_one_padded_column aside: its point is the one padded column), and at least two of the pairs
(stride, pad0, pad1, dilation, kernel) differ between the axes wherever the case is not a named TF layer."""
from helpers import conv_geom


def G(k, s, pads, d=(1, 1)):
    return dict(kh=k[0], kw=k[1], sh=s[0], sw=s[1], ph0=pads[0], ph1=pads[1], pw0=pads[2], pw1=pads[3], dh=d[0], dw=d[1])


RELU, RELU6, NONE = 0, 6, -1

# group-1 convolutions on an inner (NHWC on the device) tensor: the int8 GEMM family, conv_u8_*, conv_f32_mfma
GEMM = {
    "tf_same_s2": (2, 24, 11, 14, 40, 1, RELU, G((3, 3), (2, 2), (0, 1, 0, 1))),
    "stride_h_only": (1, 32, 12, 9, 48, 1, RELU6, G((3, 3), (2, 1), (1, 1, 1, 1))),
    "row_kernel": (3, 16, 7, 19, 24, 1, NONE, G((1, 5), (1, 3), (0, 0, 2, 1))),
    "dilation_differs": (1, 32, 12, 17, 48, 1, RELU, G((3, 2), (1, 1), (2, 1, 0, 3), (2, 3))),
    "pw_stride_w": (3, 64, 7, 10, 64, 1, RELU, G((1, 1), (1, 2), (0, 0, 0, 0))),                  # 1x1 but not the planners' is1x1
    "pw_one_padded_column": (1, 32, 6, 5, 32, 1, RELU, G((1, 1), (1, 1), (0, 0, 0, 1))),          # last column = the requantised bias
    "pw_tf_same_s2": (2, 64, 7, 10, 64, 1, RELU, G((1, 1), (2, 2), (0, 1, 0, 1))),                # strided 1x1 whose last column lies in the pad
    "k64_two_groups": (2, 64, 10, 13, 128, 1, RELU, G((3, 3), (1, 2), (1, 0, 0, 1))),             # cin % 64 == 0: the pgemm variants
    "taller_than_image": (1, 8, 3, 6, 8, 1, RELU, G((5, 3), (1, 1), (2, 2, 1, 0))),
}

# depthwise 3x3 with stride_h == stride_w: the dwconv3x3 launch (int8), with either depthwise formula
DW3X3 = {
    "dw_tf_same_s2_b1": (1, 48, 15, 12, 48, 48, RELU, G((3, 3), (2, 2), (0, 1, 0, 1))),           # batch 1, pads not pairwise equal: the REF formula
    "dw_ph_ne_pw_b1": (1, 32, 9, 14, 32, 32, RELU, G((3, 3), (1, 1), (1, 1, 0, 0))),              # pairwise equal: the HCL formula, PH != PW
    "dw_ragged_b3": (3, 40, 8, 11, 40, 40, RELU, G((3, 3), (1, 1), (1, 0, 0, 1))),
}

# depthwise / grouped shapes outside the 3x3 launch: conv_direct_i8, conv_u8_direct, conv_f32_direct
DIRECT = {
    "dw_stride_2_1": (1, 24, 11, 8, 24, 24, RELU, G((3, 3), (2, 1), (1, 1, 1, 1))),
    "dw_3x5_dil_1_2": (2, 16, 9, 13, 16, 16, RELU, G((3, 5), (1, 1), (1, 1, 4, 4), (1, 2))),
    "grouped_2x3": (3, 12, 8, 10, 12, 4, RELU, G((2, 3), (1, 2), (1, 0, 0, 2))),
}

# the graph's first layer, read from the NCHW input
FIRST = {
    "first_3x3_s21": (1, 3, 21, 26, 32, 1, RELU, G((3, 3), (2, 1), (0, 1, 1, 0))),
    "first_7x5_s23": (1, 3, 30, 33, 16, 1, RELU, G((7, 5), (2, 3), (3, 2, 2, 1))),
    "first_dil_2_1": (2, 4, 17, 12, 24, 1, RELU, G((3, 3), (1, 1), (2, 2, 1, 1), (2, 1))),
    "first_8ch_3x2": (1, 8, 9, 12, 16, 1, RELU, G((3, 2), (2, 1), (1, 0, 0, 1))),                 # cin > 4: not the first-layer kernel's
}

# SAME pad codes in pad_h0 / pad_w0 (-1: smaller half first, -2: larger half first; resolved by infer_shape, convolution.c:76-121).
# Stride 2 on 10x13 (pad_num 1 | 2) and on 11x14 (2 | 1) with kernel 3, (3 | 4) and (4 | 3) with kernel 5; dilation is not in pad_num
SAME = {
    "same_k3_s2_even_upper": (2, 16, 10, 13, 24, 1, RELU, G((3, 3), (2, 2), (-1, 0, -1, 0))),
    "same_k3_s2_odd_lower": (1, 16, 11, 14, 24, 1, RELU, G((3, 3), (2, 2), (-2, 0, -2, 0))),
    "same_k5_s2_even_upper_lower": (1, 16, 10, 13, 24, 1, RELU, G((5, 5), (2, 2), (-1, 0, -2, 0))),
    "same_k5_s2_odd_lower_upper": (2, 16, 11, 14, 24, 1, RELU, G((5, 5), (2, 2), (-2, 0, -1, 0))),
    "same_k3_s21_dil2": (1, 16, 11, 14, 24, 1, RELU, G((3, 3), (2, 1), (-2, 0, -1, 0), (2, 2))),
    "same_dw_s2_b1": (1, 32, 10, 13, 32, 32, RELU, G((3, 3), (2, 2), (-1, 0, -1, 0))),             # resolves to 0,1 / 1,1: the REF formula at batch 1
}

# fp32 only: 3x3 / stride 1 with pads that differ, forced through the device's Winograd F(2,3)
F32_WINO = {
    "wino_p0110": (2, 16, 9, 12, 32, 1, RELU, G((3, 3), (1, 1), (0, 1, 1, 0))),
    "wino_p2011": (1, 33, 15, 14, 70, 1, RELU6, G((3, 3), (1, 1), (2, 0, 1, 1))),
}

CONV_TABLES = dict(gemm=GEMM, dw3x3=DW3X3, direct=DIRECT, first=FIRST, same=SAME)
ALL_CONV = {"%s/%s" % (t, k): v for t, tab in CONV_TABLES.items() for k, v in tab.items()}

# pools: (n, c, h, w, alg (0 max, 1 avg), caffe, geom); a pool's shape follows pad_*0 alone (pooling.c:69-78)
def P(k, s, pads):
    return dict(kh=k[0], kw=k[1], sh=s[0], sw=s[1], ph0=pads[0], ph1=pads[0], pw0=pads[1], pw1=pads[1])


POOLS = {
    "max_3x2_s21_p10": (2, 16, 11, 14, 0, 0, P((3, 2), (2, 1), (1, 0))),
    "avg_2x3_s12_p01": (2, 16, 11, 14, 1, 0, P((2, 3), (1, 2), (0, 1))),
    "avg_2x3_s12_p01_caffe": (2, 16, 11, 14, 1, 1, P((2, 3), (1, 2), (0, 1))),
    "max_3x3_s2_p01_odd": (1, 24, 13, 9, 0, 0, P((3, 3), (2, 2), (0, 1))),
}


TF_S2 = G((3, 3), (2, 2), (0, 1, 0, 1))       # the stride-2 layer of a TF-converted model, convolution or depthwise


def fused_graph(name, n):
    """(graph, input) of an int8 multi-node case at batch n: the shapes the fused launches take (or must refuse)"""
    from block_helpers import block_graph
    from helpers import dwpw_graph, pwdw_graph, stem_graph
    from test_gpu_chain4 import chain_graph
    from yolo_i8_helpers import relu_pool_graph
    seed = seed_of(name) + n
    chain_dw = {"dw1": G((3, 3), (1, 1), (0, 1, 1, 0)), "dw2": TF_S2}
    pool = P((3, 2), (2, 1), (1, 0))
    if name == "firstdw_tf_stem":              # TF MobileNet stem: conv 3x3 s2 (0,1,0,1) -> dw s1 pad 1
        return pwdw_graph(seed, n, 3, 21, 18, 32, first=(3, 2, 0), first_geom=TF_S2, dw_geom=G((3, 3), (1, 1), (1, 1, 1, 1)))
    if name == "firstdw_tf_stem_same":         # the same pair written with the SAME code
        return pwdw_graph(seed, n, 3, 21, 18, 32, first=(3, 2, 0), first_geom=G((3, 3), (2, 2), (-1, 0, -1, 0)), dw_geom=G((3, 3), (1, 1), (-1, 0, -1, 0)))
    if name == "firstdw_3x4_dilh2":
        return pwdw_graph(seed, n, 3, 23, 17, 24, first=(3, 1, 0), first_geom=G((3, 4), (2, 1), (1, 1, 2, 1), (2, 1)), dw_geom=TF_S2)
    if name == "pwdw_tf_s2":
        return pwdw_graph(seed, n, 32, 11, 14, 64, dw_geom=TF_S2)
    if name == "pwdw_s1_p2012":
        return pwdw_graph(seed, n, 24, 9, 7, 40, dw_geom=G((3, 3), (1, 1), (2, 0, 1, 2)))
    if name == "dwpw_p1001":                   # (64 outputs: dwpw.hip takes whole 64-channel wave slices only)
        return dwpw_graph(seed, n, 48, 10, 13, 64, dw_geom=G((3, 3), (1, 1), (1, 0, 0, 1)))
    if name == "chain_pw":
        return chain_graph(seed, n, 32, 13, 10, 48, 40, 2, geoms=chain_dw)
    if name == "chain_first":
        return chain_graph(seed, n, 3, 27, 21, 24, 40, 2, first=(3, 2, 0), geoms=dict(chain_dw, prod=TF_S2))
    if name == "block_p2011":                  # keeps the map size, but is not the block kernel's geometry
        return block_graph(seed, n, 64, 9, 12, 16, geom_b=G((3, 3), (1, 1), (2, 0, 1, 1)))
    if name == "stem_pool_3x2":
        return stem_graph(seed, n, 37, 29, 32, pool_g=pool, caffe=0)
    if name == "relu_pool_3x2":
        return relu_pool_graph(seed, (n, 16, 11, 14), 0, 0, 0, 0, 0.1, 0.03, 0.041, 0.05, geom=pool)
    raise KeyError(name)


# name -> batches
FUSED = {"firstdw_tf_stem": (1, 2), "firstdw_tf_stem_same": (1, 2), "firstdw_3x4_dilh2": (1, 2), "pwdw_tf_s2": (1, 3), "pwdw_s1_p2012": (1, 3),
         "dwpw_p1001": (2,), "chain_pw": (1, 2), "chain_first": (1, 2), "block_p2011": (2,), "stem_pool_3x2": (1,), "relu_pool_3x2": (2,)}


def seed_of(name):
    """a fixed seed per case name (the tables may grow without moving the others' seeds)"""
    return SEEDS.get(name, 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 1000)


# seeds chosen so that the expected output passes not_degenerate (relu6 leaves 6 / out_scale + 1 levels: a small input scale is needed)
SEEDS = {"gemm/stride_h_only": 2}


def asymmetric(geom):
    g = conv_geom(geom)
    return g["ph0"] >= 0 and g["pw0"] >= 0 and (g["ph0"] != g["ph1"] or g["pw0"] != g["pw1"])


def not_degenerate(want):
    """the guard test_gpu_chain4.py uses: a graph whose output is (nearly) constant cannot pass for parity"""
    import numpy as np
    return len(np.unique(want)) >= 16 and np.count_nonzero(want == 0) < 0.8 * want.size
