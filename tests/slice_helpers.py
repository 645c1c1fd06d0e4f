"""Graphs that hand an int8 operator a channel SLICE on the side it reads, on the side it writes, or both -- what the planner does
whenever it removes a channel Concat (graph_plan.hip: plan_concat_views) -- shared by tests/test_slices_cpu.py (the conditions on the
inputs, checked with the oracle on the CPU) and the tests/test_gpu_slices_*.py files (the device against the oracle / the reference).

    data [n,16,h,w]
      |- conv1x1 -> part 0 -|
      |- conv1x1 -> part 1 -|  Concat "mid", every part at mid's scale: the parts are views of mid, mid is graph output 0
      |- conv1x1 -> part 2 -|
      OP UNDER TEST reads one part (in_slice = (offset, width, cs)) -> t
      neighbour conv1x1 (reads ANOTHER part) -> nb         (one in front of t where t's offset is not 0, one behind where room is left)
      Concat "out" of [nb.., t, nb..], all at one scale -> graph output 1      (out_slice = (offset, ldc))

An input slice in the middle of mid has a part on either side of it; one at an end has one neighbour.  The operator's node is named
"op" (a chain of nodes: "op", "op1", ..), so a test finds its launch in the profile by that name."""
import numpy as np

from helpers import _scales
from tengine_amd import tm2
from tengine_amd.tm2 import DT_INT8, DT_INT32, Graph

# standard deviation of a convolution's outputs in steps of its output scale: 45 keeps |q| = 127 at about half a percent
SPREAD = 45.0


def conv_out(i, k, s, p):
    return (i + 2 * p - k) // s + 1


def add_conv(g, rng, name, x, cin, cout, n, h, w, out_scale, k=1, sh=1, sw=1, p=0, group=1, act=-1, bias=True, fit=False):
    """one Convolution node behind tensor x ([n, cin, h, w]); returns (output tensor, oh, ow).  fit: the weight scales are sized to
    out_scale (a neighbour, whose output scale is the operator's), so that its outputs spread like everyone else's"""
    wq = rng.integers(-127, 128, size=(cout, cin // group, k, k)).astype(np.int8)
    ws = _scales(rng, cout, 0.006, 0.016)          # (mean 0.011: walk)
    if fit:
        m = out_scale / (g.tensors[x].scales[0] * 0.011 * 73.0 * np.sqrt((cin // group) * k * k))
        ws = [float(np.float32(v * m)) for v in ws]
    ins = [x, g.add_const(name + "_w", wq, DT_INT8, ws, [0] * cout)]
    if bias:
        ins.append(g.add_const(name + "_b", rng.integers(-2000, 2000, size=(cout,)).astype(np.int32), DT_INT32, [1.0], [0]))
    oh, ow = conv_out(h, k, sh, p), conv_out(w, k, sw, p)
    y = g.add_tensor(name, [n, cout, oh, ow], DT_INT8, tm2.TT_VAR, None, [out_scale], [0])
    g.add_node(name, "Convolution", ins, [y], kernel_h=k, kernel_w=k, stride_h=sh, stride_w=sw, dilation_h=1, dilation_w=1,
               input_channel=cin, output_channel=cout, group=group, activation=act, pad_h0=p, pad_w0=p, pad_h1=p, pad_w1=p)
    return y, oh, ow


def add_pool(g, name, x, c, n, h, w, out_scale, alg=0, k=2, s=2, p=0, glob=0, caffe=0):
    from helpers import pool_geom, pool_geom_out, pool_geom_params
    G = pool_geom(None, k, s, p)
    if glob:
        G.update(kh=h, kw=w)
    oh, ow = pool_geom_out(h, w, G, glob, caffe)
    y = g.add_tensor(name, [n, c, oh, ow], DT_INT8, tm2.TT_VAR, None, [out_scale], [0])
    g.add_node(name, "Pooling", [x], [y], alg=alg, **{"global": glob}, caffe_flavor=caffe, **pool_geom_params(G))
    return y, oh, ow


def _stride_for(i, o):
    """the stride at which a 1x1 convolution turns extent i into extent o"""
    for s in range(1, i + 1):
        if (i - 1) // s + 1 == o:
            return s
    raise AssertionError("no 1x1 stride maps %d to %d" % (i, o))


def front(g, rng, n, h, w, widths):
    """data -> one 1x1 convolution per width -> Concat "mid"; returns (part tensors, mid's node index, mid's scale)"""
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    x = g.add_input("data", [n, 16, h, w], DT_INT8, [xs], [0])
    ms = float(np.float32(xs * 0.011 * 73.0 * 4.0 * 73.0 / SPREAD))
    parts = [add_conv(g, rng, "part%d" % i, x, 16, c, n, h, w, out_scale=ms)[0] for i, c in enumerate(widths)]
    mid = g.add_tensor("mid", [n, sum(widths), h, w], DT_INT8, tm2.TT_VAR, None, [ms], [0])
    return parts, g.add_node("mid", "Concat", parts, [mid], axis=1), ms


def split_widths(in_slice):
    """(widths of mid's parts, index of the part the operator reads)"""
    off, width, cs = in_slice
    assert off % 16 == 0 and width % 16 == 0 and cs % 16 == 0 and 0 < width and off + width <= cs and width < cs
    widths = [c for c in (off, width, cs - off - width) if c]
    return widths, 1 if off else 0


def _chain(op):
    return op if isinstance(op, list) else [op]


def walk(op, cin, h, w, ms):
    """what the operator (a dict of kind "conv" | "pool", or a list of them: a chain) makes of a [., cin, h, w] tensor of scale ms:
    (the output scale of every node, cout, oh, ow).  A convolution's scale follows from its fan-in (add_conv), a pool's is its
    `scale_mul` times its input's: sized so that the outputs use the int8 range and few saturate"""
    from helpers import pool_geom, pool_geom_out
    scales, c, s = [], cin, ms
    for o in _chain(op):
        if o["kind"] == "conv":
            k = o.get("k", 1)
            fan = k * k * (1 if o.get("depthwise") else c // o.get("group", 1))
            s = float(np.float32(s * 0.011 * 73.0 * np.sqrt(fan) * o.get("scale_mul", 1.0)))
            c = o.get("cout", c)
            h, w = conv_out(h, k, o.get("sh", 1), o.get("p", 0)), conv_out(w, k, o.get("sw", 1), o.get("p", 0))
        else:
            assert o["kind"] == "pool", o
            s = float(np.float32(s * o["scale_mul"]))
            G = pool_geom(None, o.get("k", 2), o.get("s", 2), o.get("p", 0))
            if o.get("glob"):
                G.update(kh=h, kw=w)
            h, w = pool_geom_out(h, w, G, o.get("glob", 0), o.get("caffe", 0))
        scales.append(s)
    return scales, c, h, w


def add_op(g, rng, op, x, cin, n, h, w, ms, prefix="op"):
    """the operator under test behind tensor x, its nodes named "op", "op1", ..; returns the output tensor"""
    scales = walk(op, cin, h, w, ms)[0]
    c = cin
    for i, o in enumerate(_chain(op)):
        name = prefix if i == 0 else "%s%d" % (prefix, i)
        o = dict(o)
        if o.pop("kind") == "conv":
            cout = o.pop("cout", c)
            o.pop("scale_mul", None)
            if o.pop("depthwise", False):
                o["group"] = c
            x, h, w = add_conv(g, rng, name, x, c, cout, n, h, w, out_scale=scales[i], **o)
            c = cout
        else:
            o.pop("scale_mul")
            x, h, w = add_pool(g, name, x, c, n, h, w, scales[i], **o)
    return x


def slice_graph(seed, n, h, w, op, in_slice, out_slice, run_last=True):
    """see the module text.  in_slice = (offset, width, cs) of the tensor the operator reads, out_slice = (offset, ldc) of the one it
    writes (its width is the operator's); run_last: the operator's nodes stand BEHIND its output neighbours, so that its launch runs
    after theirs and bytes it writes outside its slice destroy what the comparison sees"""
    rng = np.random.default_rng(seed)
    g = Graph(name="slice_case")
    widths, mine = split_widths(in_slice)
    parts, mid_node, ms = front(g, rng, n, h, w, widths)
    others = [i for i in range(len(parts)) if i != mine]
    o_off, ldc = out_slice
    scales, cout, oh, ow = walk(op, widths[mine], h, w, ms)
    assert o_off % 16 == 0 and ldc % 16 == 0 and cout % 16 == 0 and o_off + cout <= ldc and cout < ldc, (out_slice, cout)

    def neighbours():
        nbs = {}
        for j, c in enumerate((o_off, ldc - o_off - cout)):
            if c:
                src = others[j % len(others)]
                nbs[j] = add_conv(g, rng, "nb%d" % j, parts[src], widths[src], c, n, h, w, out_scale=scales[-1], sh=_stride_for(h, oh),
                                  sw=_stride_for(w, ow), fit=True)[0]
        return nbs

    if run_last:
        nbs = neighbours()
        t = add_op(g, rng, op, parts[mine], widths[mine], n, h, w, ms)
    else:
        t = add_op(g, rng, op, parts[mine], widths[mine], n, h, w, ms)
        nbs = neighbours()
    ins = [nbs[j] for j in (0,) if j in nbs] + [t] + [nbs[j] for j in (1,) if j in nbs]
    out = g.add_tensor("out", [n, ldc, oh, ow], DT_INT8, tm2.TT_VAR, None, [scales[-1]], [0])
    g.output_nodes = [mid_node, g.add_node("out", "Concat", ins, [out], axis=1)]
    return g, rng.integers(-127, 128, size=(n, 16, h, w)).astype(np.int8)


def slice_eltwise_graph(seed, n, h, w, op, in_slice):
    """conv (the operator, reading its slice of mid) -> Eltwise SUM with a second convolution of the same geometry on ANOTHER part of
    mid -> ReLU: the ResNet block tail that the GEMM family folds into its epilogue.  The tail's tensors are dense (the planner makes
    no Eltwise operand a view); outputs: mid, the ReLU"""
    rng = np.random.default_rng(seed)
    g = Graph(name="slice_eltwise_case")
    widths, mine = split_widths(in_slice)
    parts, mid_node, ms = front(g, rng, n, h, w, widths)
    other = [i for i in range(len(parts)) if i != mine][0]
    op = dict(op, act=-1)
    (sa,), cout, oh, ow = walk(op, widths[mine], h, w, ms)
    sb = float(np.float32(sa * 1.37))
    kw = {k: v for k, v in op.items() if k not in ("kind", "cout")}
    b = add_conv(g, rng, "other", parts[other], widths[other], cout, n, h, w, out_scale=sb, fit=True, **kw)[0]      # the EARLIER producer
    a = add_op(g, rng, op, parts[mine], widths[mine], n, h, w, ms)
    so = float(np.float32(sa * 1.9))
    e = g.add_tensor("sum", [n, cout, oh, ow], DT_INT8, tm2.TT_VAR, None, [so], [0])
    g.add_node("elt", "Eltwise", [a, b], [e], type=tm2.ELT_SUM, caffe_flavor=1)
    r = g.add_tensor("relu", [n, cout, oh, ow], DT_INT8, tm2.TT_VAR, None, [so], [0])
    g.output_nodes = [mid_node, g.add_node("relu", "ReLU", [e], [r], negative_slope=0.0)]
    return g, rng.integers(-127, 128, size=(n, 16, h, w)).astype(np.int8)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# id: (h, w, operator, input slice (offset, width, cs), output slice (offset, ldc)); all at n = 2 (the image stride N * H * W * cs_in)
GEMM_SHAPES = {
    # 1x1 on 33 x 33: M = 2178 is ragged in 32 / 64 / 128; cout 80 > 64 reaches the 128-wide pgemm rows
    "pw_many": (33, 33, dict(kind="conv", cout=80, k=1, act=0), (32, 64, 96), (16, 96)),
    # 1x1 on 7 x 9: M = 126 (gemm_direct, pw_small, the 64-pixel pgemm tiles)
    "pw_few": (7, 9, dict(kind="conv", cout=16, k=1), (16, 32, 48), (32, 48)),
    # 3x3 on 64 channels: ckp % 64 == 0 (conv_pgemm_w, the igemm fast loader), kpad 576 (igemm 5 - 9)
    "k3": (12, 10, dict(kind="conv", cout=32, k=3, p=1, act=6), (64, 64, 128), (32, 64)),
    # 3x3 / 2 on 16 channels: the generic loaders (ckp 16, kpad 192 > ktot 144)
    "k3_s2_c16": (9, 7, dict(kind="conv", cout=16, k=3, sh=2, sw=2, p=1), (16, 16, 32), (0, 48)),
    # M = 8192: conv_igemm2's 64 blocks of 128 pixels -- the smallest M that gives it them
    "big": (64, 64, dict(kind="conv", cout=32, k=3, p=1, act=0), (16, 16, 32), (16, 48)),
    # not in the issue's table: the 128 x 128 conv_pgemm_w forms need more than 64 output channels on a 3 x 3 layer of 64-channel groups
    "k3_wide": (12, 10, dict(kind="conv", cout=80, k=3, p=1), (64, 64, 128), (16, 96)),
}
# the dedicated 3 x 3 forms of conv_pgemm_w.hip by their full names (the family list of test_gpu_gemm_family.py names tile sizes only)
PGEMM_W_MEMBERS = {
    "conv_pgemm_i8<128x64,3x3,w4t>": "k3", "conv_pgemm_i8<128x64,3x3,w4b3>": "k3", "conv_pgemm_i8<64x64,3x3,w4t>": "k3",
    "conv_pgemm_i8<64x64,3x3,w4b3>": "k3", "conv_pgemm_i8<128x128,3x3,w8>": "k3_wide", "conv_pgemm_i8<128x128,3x3,w8b3>": "k3_wide",
}
SEED = 7100


def gemm_case(shape, run_last):
    h, w, op, ins, outs = GEMM_SHAPES[shape]
    return slice_graph(SEED + sorted(GEMM_SHAPES).index(shape), 2, h, w, op, ins, outs, run_last)


def gemm_eltwise_case(shape):
    h, w, op, ins, _ = GEMM_SHAPES[shape]
    return slice_eltwise_graph(SEED + 50 + sorted(GEMM_SHAPES).index(shape), 2, h, w, op, ins)


# ---- the byte -128 through every in-place producer ------------------------------------------------------------------------------
# The reference's int8 Concat of several inputs stores 127 for -128, even between equal scales (concat_kernel_ref_int8.c:83-84).  A
# producer that writes its output in place of the Concat's copy has to store what that copy would have.
CAT_SCALE = 0.05
MAP_SCALE = 0.03      # bytes 213 and 214 map to 128 at the ratio 0.6: round(213 * 0.6) = round(127.8), round(214 * 0.6) = round(128.4)
# id: (producer, the input's scale, n, the producer's tensor first?, channels of the side convolution, who the side convolution reads)
# "own": the side convolution reads the producer's tensor p, which must hold -128 for it while the Concat's readers see 127: one buffer
# cannot be both, so an Upsample with a second reader is copied by concat_copy_i8 (1 copy); "twin": it reads a second producer of the same
# kind, the Concat is p's only reader and p is written in place (no copy)
MINUS128_CASES = {
    "upsample_copy": ("upsample", CAT_SCALE, 1, True, 16, "own"),
    "upsample_copy_second": ("upsample", CAT_SCALE, 1, False, 16, "own"),
    "upsample_map": ("upsample", MAP_SCALE, 1, True, 16, "own"),
    "upsample_map_second": ("upsample", MAP_SCALE, 1, False, 16, "own"),
    "upsample_copy_batch2_offset48": ("upsample", CAT_SCALE, 2, False, 48, "own"),
    "upsample_map_batch2_offset48": ("upsample", MAP_SCALE, 2, False, 48, "own"),
    "upsample_copy_sole_reader": ("upsample", CAT_SCALE, 1, True, 16, "twin"),
    "upsample_copy_sole_reader_second": ("upsample", CAT_SCALE, 1, False, 16, "twin"),
    "upsample_map_sole_reader": ("upsample", MAP_SCALE, 1, True, 16, "twin"),
    "upsample_map_sole_reader_second": ("upsample", MAP_SCALE, 1, False, 16, "twin"),
    "upsample_copy_sole_reader_batch2_offset48": ("upsample", CAT_SCALE, 2, False, 48, "twin"),
    "upsample_map_sole_reader_batch2_offset48": ("upsample", MAP_SCALE, 2, False, 48, "twin"),
    "pool_max": ("pool", CAT_SCALE, 1, True, 16, "own"),
    "pool_max_second": ("pool", CAT_SCALE, 2, False, 48, "own"),
    "interp_nearest": ("interp", CAT_SCALE, 1, True, 16, "own"),
    "interp_nearest_second": ("interp", CAT_SCALE, 2, False, 48, "own"),
}


def minus128_copies(case):
    """concat_copy_i8 launches the planner owes the case (see above)"""
    return 1 if MINUS128_CASES[case][0] == "upsample" and MINUS128_CASES[case][5] == "own" else 0


def minus128_graph(case):
    """data [n,16,4,4] holding every byte value -> Upsample x2 (nearest Interp x2; for the pool: data [n,16,16,16] -> MAX 2x2 / 2) -> p;
    Concat of [p, conv1x1(p)] or of [conv1x1(p), p], every tensor at the Concat's scale ("twin": the convolution reads a second
    producer of the same kind)"""
    from interp_helpers import by_scale
    from yolo_i8_helpers import all_bytes_inputs
    producer, s_in, n, first, side, reads = MINUS128_CASES[case]
    rng = np.random.default_rng(7300 + sorted(MINUS128_CASES).index(case))
    g = Graph(name="minus128_case")
    cs = float(np.float32(CAT_SCALE))
    dims = [n, 16, 16, 16] if producer == "pool" else [n, 16, 4, 4]
    x = g.add_input("data", dims, DT_INT8, [float(np.float32(s_in))], [0])

    def produce(name):
        if producer == "pool":
            return add_pool(g, name, x, 16, n, 16, 16, cs, alg=0, k=2, s=2)[0]
        t = g.add_tensor(name, [n, 16, 8, 8], DT_INT8, tm2.TT_VAR, None, [cs], [0])
        if producer == "upsample":
            g.add_node(name, "Upsample", [x], [t], scale=2.0)
        else:
            g.add_node(name, "Interp", [x], [t], **by_scale(2.0))
        return t

    p = produce("op")
    c = add_conv(g, rng, "side", p if reads == "own" else produce("twin"), 16, side, n, 8, 8, out_scale=cs, fit=True)[0]
    y = g.add_tensor("cat", [n, 16 + side, 8, 8], DT_INT8, tm2.TT_VAR, None, [cs], [0])
    g.output_nodes = [g.add_node("cat", "Concat", [p, c] if first else [c, p], [y], axis=1)]
    xin = all_bytes_inputs(7300, dims)[0].copy()
    if producer == "pool":                           # windows of nothing but -128: their maximum is -128
        xin[:, :, 0:2, 0:4] = -128
        xin[:, 3:9, 6:8, 10:12] = -128
    elif n > 1:                                      # room beside the 256 byte values: a second and third -128 per tensor
        flat = xin.reshape(-1)
        vals, counts = np.unique(flat, return_counts=True)
        for v in vals[(counts > 1) & (vals != -128)][:2]:      # in place of a value that occurs twice: every byte value stays
            flat[np.flatnonzero(flat == v)[0]] = -128
    return g, xin


def upsample_bytes(x, s_in, s_out, factor=2):
    """upsample_ref.c's uint8 routine on the int8 BYTES, restated: u = 0 .. 255, round(u * s_in / s_out) clamped to 0 .. 255, stored
    into the int8 tensor; equal scales: the bytes as they are"""
    u = x.view(np.uint8).astype(np.float32)
    if np.float32(s_in) != np.float32(s_out):
        v = (u * np.float32(s_in)) / np.float32(s_out)
        u = np.clip(np.floor(v + np.float32(0.5)), 0, 255)
    q = u.astype(np.uint8).view(np.int8)
    return np.repeat(np.repeat(q, factor, 2), factor, 3)


# ---- the other int8 launchers ---------------------------------------------------------------------------------------------------
OPS_IN, OPS_OUT = (16, 32, 64), (32, 80)          # slices of the cases below unless a case names its own


def dw_case(form_stride, run_last):
    """depthwise 3x3, pad 1, on a 9 x 11 map (one of the ten forms of dwconv.hip, pinned by the test)"""
    return slice_graph(7400 + form_stride, 2, 9, 11, dict(kind="conv", k=3, sh=form_stride, sw=form_stride, p=1, depthwise=True, act=0), OPS_IN, OPS_OUT, run_last)


# id: (h, w, operator, input slice, output slice, kernel name of node "op")
OP_CASES = {
    "direct_group2_3x3": (9, 11, dict(kind="conv", cout=32, k=3, p=1, group=2), OPS_IN, OPS_OUT, "conv_direct_i8"),
    "direct_depthwise_5x5": (9, 11, dict(kind="conv", k=5, p=2, depthwise=True), (16, 16, 64), OPS_OUT, "conv_direct_i8"),
    "pool_max_3x3_s2_p1": (10, 12, dict(kind="pool", alg=0, k=3, s=2, p=1, scale_mul=1.3), OPS_IN, OPS_OUT, "pool_i8"),
    "pool_avg_2x2_s2": (10, 12, dict(kind="pool", alg=1, k=2, s=2, scale_mul=0.55), OPS_IN, OPS_OUT, "pool_i8"),
    "pool_max_caffe_flavor": (10, 12, dict(kind="pool", alg=0, k=3, s=2, caffe=1, scale_mul=1.3), OPS_IN, OPS_OUT, "pool_i8"),
    "global_max_5x13": (5, 13, dict(kind="pool", alg=0, glob=1, scale_mul=1.7), OPS_IN, OPS_OUT, "pool_i8"),
    "global_avg_5x13": (5, 13, dict(kind="pool", alg=1, glob=1, scale_mul=0.13), OPS_IN, OPS_OUT, "pool_i8"),
    "global_max_1x1": (1, 1, dict(kind="pool", alg=0, glob=1, scale_mul=1.1), OPS_IN, OPS_OUT, "pool_i8"),
    "global_avg_1x1": (1, 1, dict(kind="pool", alg=1, glob=1, scale_mul=0.9), OPS_IN, OPS_OUT, "pool_i8"),
}


# seeds moved on where the 128 bytes of a 1 x 1 map happened to hold too many +-127 (tests/test_slices_cpu.py states the condition)
SEED_SHIFT = {"global_avg_1x1": 101}


def op_case(case, run_last):
    h, w, op, ins, outs, _ = OP_CASES[case]
    return slice_graph(7500 + sorted(OP_CASES).index(case) + SEED_SHIFT.get(case, 0), 2, h, w, op, ins, outs, run_last)


def first_graph(seed, n, h, w, k, p, cout, ldc, offset, pool, run_last):
    """the first-layer convolution (3 channels from an NCHW graph input, k x k / 2) [-> MAX pool 3x3 / 2] with its output a view: one
    such stem per graph input (a graph input with a second reader is staged as NHWC and takes the GEMM family instead), all into one
    Concat.  Every input of the graph takes the same array.  Nodes "op" [, "op1"]: the stem at `offset`"""
    rng = np.random.default_rng(seed)
    g = Graph(name="first_slice_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    ms = float(np.float32(xs * 0.011 * 73.0 * np.sqrt(3 * k * k) * 73.0 / SPREAD))
    os_ = float(np.float32(ms * 1.25)) if pool else ms         # (a maximum of nine lies higher than its inputs)
    widths = [c for c in (offset, cout, ldc - offset - cout) if c]
    mine = 1 if offset else 0
    order = [i for i in range(len(widths)) if i != mine]
    order = order + [mine] if run_last else [mine] + order
    outs = {}
    for i in order:
        x = g.add_input("data%d" % i, [n, 3, h, w], DT_INT8, [xs], [0])
        name = "op" if i == mine else "nb%d" % i
        t, oh, ow = add_conv(g, rng, name, x, 3, widths[i], n, h, w, out_scale=ms, k=k, sh=2, sw=2, p=p, act=0)
        if pool:
            t, oh, ow = add_pool(g, "op1" if i == mine else name + "_pool", t, widths[i], n, oh, ow, os_, alg=0, k=3, s=2, caffe=1)
        outs[i] = t
    y = g.add_tensor("out", [n, ldc, oh, ow], DT_INT8, tm2.TT_VAR, None, [os_], [0])
    g.output_nodes = [g.add_node("out", "Concat", [outs[i] for i in range(len(widths))], [y], axis=1)]
    return g, rng.integers(-127, 128, size=(n, 3, h, w)).astype(np.int8), len(widths)


# id: (h, w, k, pad, cout, ldc, offset, pool, kernel name)
FIRST_CASES = {
    "first_3x3_s2": (17, 19, 3, 1, 16, 48, 16, False, "conv_first_i8"),
    "first_7x7_s2_pool": (37, 41, 7, 3, 16, 48, 16, True, "conv_first_pool_i8"),
}


def first_case(case, run_last):
    h, w, k, p, cout, ldc, off, pool, _ = FIRST_CASES[case]
    return first_graph(7600 + sorted(FIRST_CASES).index(case), 2, h, w, k, p, cout, ldc, off, pool, run_last)


def fc_concat_graph(seed, second_first):
    """two FullyConnected nodes (16 -> 32, 16 -> 48) at batch 3 into a 2-D Concat, both at its scale: written in place at offsets 0 / 32
    of rows of 80.  second_first: the node of the 48-wide one stands first"""
    rng = np.random.default_rng(seed)
    g = Graph(name="fc_slice_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    x = g.add_input("data", [3, 16], DT_INT8, [xs], [0])
    os_ = float(np.float32(xs * 0.011 * 73.0 * 4.0 * 73.0 / SPREAD))
    outs = {}
    for i in ((1, 0) if second_first else (0, 1)):
        nout = (32, 48)[i]
        ins = [x, g.add_const("w%d" % i, rng.integers(-127, 128, size=(nout, 16)).astype(np.int8), DT_INT8, _scales(rng, nout, 0.006, 0.016), [0] * nout),
               g.add_const("b%d" % i, rng.integers(-2000, 2000, size=(nout,)).astype(np.int32), DT_INT32, [1.0], [0])]
        outs[i] = g.add_tensor("fc%d" % i, [3, nout], DT_INT8, tm2.TT_VAR, None, [os_], [0])
        g.add_node("fc%d" % i, "FullyConnected", ins, [outs[i]], num_output=nout)
    y = g.add_tensor("out", [3, 80], DT_INT8, tm2.TT_VAR, None, [os_], [0])
    g.output_nodes = [g.add_node("out", "Concat", [outs[0], outs[1]], [y], axis=1)]
    return g, rng.integers(-127, 128, size=(3, 16)).astype(np.int8)


# ---- uint8: a convolution writes a channel range of the Concat's NCHW buffer (plan_nchw_buffers: out_img / out_c0) ---------------
def u8_concat_graph(seed, cin, k, cout, second, tail=None, n=2, h=5, w=7):
    """data [n, cin, h, w] -> convB (1x1, 3 channels) and -> the convolution under test ("op": k x k, pad k // 2) [-> ReLU "op1" | ->
    leaky ReLU -> MAX pool 2x2 / 2 "op2"], both into one Concat at its scale and zero point.  second: the operator's planes come
    behind convB's three, at the odd byte offset 3 * h * w of every image.  tail: None | "relu" | "pool" (a 12 x 16 map then)"""
    from helpers import _u8q
    from tengine_amd.tm2 import DT_UINT8
    rng = np.random.default_rng(seed)
    g = Graph(name="u8_slice_case")
    if tail == "pool":           # the epilogue pools even-sized maps of a multiple of 8 pixels (graph_u8.hip: find_fused_pool)
        h, w = 12, 16
    xs, xz = _u8q(rng)
    x = g.add_input("data", [n, cin, h, w], DT_UINT8, [xs], [xz])

    def conv(name, cout_, k_, q):
        ws, wz = _u8q(rng, 0.002, 0.02)
        wt = g.add_const(name + "_w", rng.integers(0, 256, size=(cout_, cin, k_, k_)).astype(np.uint8), DT_UINT8, [ws], [wz])
        bt = g.add_const(name + "_b", rng.integers(-4000, 4000, size=(cout_,)).astype(np.int32), DT_INT32, [float(np.float32(xs) * np.float32(ws))], [0])
        y = g.add_tensor(name, [n, cout_, h, w], DT_UINT8, tm2.TT_VAR, None, [q[0]], [q[1]])
        g.add_node(name, "Convolution", [x, wt, bt], [y], kernel_h=k_, kernel_w=k_, stride_h=1, stride_w=1, dilation_h=1, dilation_w=1,
                   input_channel=cin, output_channel=cout_, group=1, activation=-1, pad_h0=k_ // 2, pad_w0=k_ // 2, pad_h1=k_ // 2, pad_w1=k_ // 2)
        return y

    # one quantisation for everything that reaches the Concat; sized for the deeper of the two convolutions
    cq = (float(np.float32(xs * 0.011 * 73.0 * np.sqrt(cin * k * k) * 73.0 / 40.0)), int(rng.integers(100, 150)))
    oh, ow = h, w
    if tail is None:
        t = conv("op", cout, k, cq)
    else:
        own = (float(np.float32(cq[0] * 1.15)), int(rng.integers(100, 150)))
        t = conv("op", cout, k, own)
        slope = 0.0 if tail == "relu" else 0.1
        r = g.add_tensor("op1", [n, cout, h, w], DT_UINT8, tm2.TT_VAR, None, [cq[0]], [cq[1]])
        g.add_node("op1", "ReLU", [t], [r], negative_slope=slope)
        t = r
        if tail == "pool":
            oh, ow = h // 2, w // 2
            po = g.add_tensor("op2", [n, cout, oh, ow], DT_UINT8, tm2.TT_VAR, None, [cq[0]], [cq[1]])
            g.add_node("op2", "Pooling", [t], [po], alg=0, kernel_h=2, kernel_w=2, stride_h=2, stride_w=2, **{"global": 0}, caffe_flavor=0,
                       pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
            t = po
    if tail == "pool":       # convB on the pooled map's size: a 1x1 stride-2 convolution
        ws, wz = _u8q(rng, 0.002, 0.02)
        wt = g.add_const("convB_w", rng.integers(0, 256, size=(3, cin, 1, 1)).astype(np.uint8), DT_UINT8, [ws], [wz])
        b = g.add_tensor("convB", [n, 3, oh, ow], DT_UINT8, tm2.TT_VAR, None, [cq[0]], [cq[1]])
        g.add_node("convB", "Convolution", [x, wt], [b], kernel_h=1, kernel_w=1, stride_h=2, stride_w=2, dilation_h=1, dilation_w=1,
                   input_channel=cin, output_channel=3, group=1, activation=-1, pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
    else:
        b = conv("convB", 3, 1, cq)
    y = g.add_tensor("cat", [n, 3 + cout, oh, ow], DT_UINT8, tm2.TT_VAR, None, [cq[0]], [cq[1]])
    g.output_nodes = [g.add_node("cat", "Concat", [b, t] if second else [t, b], [y], axis=1)]
    return g, rng.integers(0, 256, size=(n, cin, h, w)).astype(np.uint8)


# conv_u8_patch.hip: conv_u8_patch_kernel_name by (configuration, kernel size); configuration 4 is the lane-level form
U8_PATCH_NAMES = {(0, 3): "conv_u8_patch_64x64<3x3>", (1, 3): "conv_u8_patch_128x64<3x3>", (2, 3): "conv_u8_patch_64x128<3x3>",
                  (3, 3): "conv_u8_patch_32x64<3x3>", (4, 3): "conv_u8_lanes<3x3>", (0, 1): "conv_u8_patch_64x64<1x1>",
                  (1, 1): "conv_u8_patch_128x64<1x1>", (2, 1): "conv_u8_patch_64x128<1x1>", (3, 1): "conv_u8_patch_32x64<1x1>",
                  (4, 1): "conv_u8_lanes<1x1>"}
# id: (pins, cin, k, cout, tail, the kernel name of node "op" starts with)
U8_CASES = {"patch%d_k%d" % (cfg, k): (dict(u8_patch=1, u8_patch_cfg=cfg), 16, k, 20, None, name) for (cfg, k), name in U8_PATCH_NAMES.items()}
U8_CASES.update({
    "pw_k32": (dict(u8_patch=0, u8_pw=1), 32, 1, 20, None, "conv_u8_pw<k32>"),
    "pw_k64": (dict(u8_patch=0, u8_pw=1), 64, 1, 20, None, "conv_u8_pw<k64>"),
    "c3_c16": (dict(u8_patch=0, u8_c3=1), 16, 3, 20, None, "conv_u8_c3<c16>"),
    "c3_c32": (dict(u8_patch=0, u8_c3=1), 32, 3, 20, None, "conv_u8_c3<c32>"),
    "rgb3x3": (dict(u8_rgb3x3=1), 3, 3, 20, None, "conv_u8_rgb3x3"),
    "default_k3": (dict(), 16, 3, 20, None, "conv_u8_"),
    "default_k1": (dict(), 24, 1, 20, None, "conv_u8_"),
    "gemm_k3": (dict(u8_patch=0, u8_c3=0), 16, 3, 20, None, "conv_u8_mfma"),
    "conv_relu": (dict(), 16, 3, 20, "relu", "conv_u8_"),
    "conv_relu_pool": (dict(), 16, 3, 20, "pool", "conv_u8_"),
    "patch_relu_pool": (dict(u8_patch=1), 16, 3, 20, "pool", "conv_u8_patch"),
    "c3_relu_pool": (dict(u8_patch=0, u8_c3=1), 16, 3, 20, "pool", "conv_u8_c3"),
})


def u8_case(case, second):
    pins, cin, k, cout, tail, _ = U8_CASES[case]
    return u8_concat_graph(7900 + sorted(U8_CASES).index(case), cin, k, cout, second, tail)


# ---- fusers next to slices -------------------------------------------------------------------------------------------------------
DW = dict(kind="conv", k=3, p=1, depthwise=True, act=0)
# id: (h, w, chain, input slice, output slice, environment, what the launch of node "op" is called where the guards let the pair fuse)
FUSER_CASES = {
    # pointwise + depthwise as one launch (pwdw.hip), the pointwise conv's INPUT a slice, the depthwise's output a view: find_pwdw_tail
    # refuses only a pointwise OUTPUT that is a view
    "pwdw_input_slice": (7, 9, [dict(kind="conv", cout=32, k=1, act=0), DW], OPS_IN, OPS_OUT, {"TAMD_FUSE_PWDW": "2"}, "pwdw_i8"),
    # depthwise + pointwise as one launch (dwpw.hip): the depthwise reads a slice, the pointwise writes 64 channels at offset 32 of 128
    # (try_dwpw refuses a depthwise OUTPUT that is a view; dwpw_applicable wants c_limit, c_off, ldc multiples of 16)
    "dwpw_both_sides": (7, 9, [DW, dict(kind="conv", cout=64, k=1, act=0)], OPS_IN, (32, 128), {"TAMD_FUSE_DWPW": "2"}, "dwpw_i8"),
}


def fuser_case(case, run_last):
    h, w, op, ins, outs, _, _ = FUSER_CASES[case]
    return slice_graph(8000 + sorted(FUSER_CASES).index(case), 2, h, w, op, ins, outs, run_last)


def chain_stem_graph(seed, run_last, n=2, h=20, w=22):
    """three stems of four layers (3x3 / 2 on the NCHW graph input -> depthwise 3x3 -> 1x1 -> depthwise 3x3: what chain4.hip runs as
    one launch), one per graph input, their last outputs (16, 32, 16 channels) views of one Concat; the middle one is "op" .. "op3".
    Every input takes the same array"""
    rng = np.random.default_rng(seed)
    g = Graph(name="chain_stem_slice_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    widths, mine = [16, 32, 16], 1
    order = [0, 2, 1] if run_last else [1, 0, 2]
    outs = {}
    for i in order:
        chain = [dict(kind="conv", cout=16, k=3, sh=2, sw=2, p=1, act=0, scale_mul=73.0 / SPREAD), dict(DW, scale_mul=0.7),
                 dict(kind="conv", cout=widths[i], k=1, act=0, scale_mul=0.7), dict(DW, scale_mul=0.7)]
        x = g.add_input("data%d" % i, [n, 3, h, w], DT_INT8, [xs], [0])
        outs[i] = add_op(g, rng, chain, x, 3, n, h, w, xs, prefix="op" if i == mine else "nb%d_" % i)
    scales, _, oh, ow = walk(chain, 3, h, w, xs)
    y = g.add_tensor("out", [n, sum(widths), oh, ow], DT_INT8, tm2.TT_VAR, None, [scales[-1]], [0])
    g.output_nodes = [g.add_node("out", "Concat", [outs[i] for i in range(3)], [y], axis=1)]
    return g, rng.integers(-127, 128, size=(n, 3, h, w)).astype(np.int8)


def block_concat_graph(seed):
    """an identity bottleneck block (block_helpers.block_graph: 1x1 -> 3x3 -> 1x1 + residual -> ReLU) whose ReLU feeds a Concat beside
    a 1x1 convolution at the same scale: a ReLU's output is no view (slice_capable), so the Concat copies it and takes the convolution
    in place"""
    from block_helpers import block_graph, tensor_index
    g, x = block_graph(seed, 2, 64, 9, 7, 16)
    rng = np.random.default_rng(seed + 1)
    out, xt = tensor_index(g, "out"), tensor_index(g, "x")
    so = g.tensors[out].scales[0]
    side = add_conv(g, rng, "side", xt, 64, 32, 2, 9, 7, out_scale=so, fit=True)[0]
    y = g.add_tensor("cat", [2, 96, 9, 7], DT_INT8, tm2.TT_VAR, None, [so], [0])
    g.output_nodes = [g.add_node("cat", "Concat", [out, side], [y], axis=1)]
    return g, x
