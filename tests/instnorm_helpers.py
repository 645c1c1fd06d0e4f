"""Builders for the tests of the uint8 InstanceNorm node (tests/test_instnorm_cpu.py, tests/test_gpu_instnorm.py,
tools/make_golden_instnorm.py): single-node graphs with chosen quantisation parameters, gamma / beta / eps and input bytes, the node in
front of a folded or unfolded ReLU, in front of a Concat and a second reader, and the generator block conv -> InstanceNorm -> ReLU -> conv
the plugin must keep whole.  Every case is tmfile bytes with explicit quantisation parameters: the reference library and the device read
the same model."""
import ctypes as C
import os

import numpy as np

import interp_helpers as ih
import lut_helpers as lh
from tengine_amd import capi, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8, Graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "instnorm_cases.npz")
OP_INSTANCENORM = 38          # TAMD_OP_INSTANCENORM
REF_OP_NAME = "InstanceNorm"  # the operator's name in the reference's op_name.h, which the plugin's placement report prints
f32 = lh.f32
equals_golden = ih.equals_golden
IN_Q, OUT_Q = (0.05, 77), (0.031, 120)
# the order-sensitive construction: large mean, small spread -- bytes 236 .. 255 at (0.0173, 0), out (6 / 255, 128), gamma 1, beta 0
ORDER_IN_Q, ORDER_OUT_Q, ORDER_SEED = (0.0173, 0), (6.0 / 255.0, 128), 3


def stats(c, seed, gamma=None, beta=None):
    """seeded gamma around 1 with both signs and beta around 0, C elements each; a number or a list overrides"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.5, 1.5, size=c) * rng.choice([-1.0, 1.0], size=c)
    b = rng.uniform(-0.5, 0.5, size=c)
    if gamma is not None:
        g = np.broadcast_to(np.asarray(gamma, np.float64), (c,))
    if beta is not None:
        b = np.broadcast_to(np.asarray(beta, np.float64), (c,))
    return g.astype(np.float32), b.astype(np.float32)


def node_graph(dtype, dims, gamma, beta, eps, in_q=IN_Q, out_q=OUT_Q, data_const=False, in_quant=None, out_quant=None, stat_dtype=DT_FP32, stat_const=True,
               inputs=3):
    """input(dims) -> InstanceNorm(gamma, beta, eps) -> output of the same dims; the keyword arguments build the nodes the rule refuses"""
    g = Graph(name="instnorm_case")
    q = lambda v: (None, None) if dtype == DT_FP32 else ([f32(v[0])], [int(v[1])])
    x = g.add_input("data", list(dims), dtype, *q(in_q))
    if in_quant is not None:
        g.tensors[x].scales, g.tensors[x].zero_points = [f32(in_q[0])] * in_quant, [int(in_q[1])] * in_quant
    src = x
    if data_const:
        src = g.add_const("table", np.zeros(dims, tm2.NP_OF_DT[dtype]), dtype, *q(in_q))
    if stat_const:
        sq = {} if stat_dtype == DT_FP32 else {"scales": [1.0], "zero_points": [0]}
        gi = g.add_const("gamma", np.asarray(gamma).astype(tm2.NP_OF_DT[stat_dtype]), stat_dtype, **sq)
        bi = g.add_const("beta", np.asarray(beta).astype(tm2.NP_OF_DT[stat_dtype]), stat_dtype, **sq)
    else:
        gi = g.add_input("gamma", [len(gamma)], DT_FP32)
        bi = g.add_input("beta", [len(beta)], DT_FP32)
    y = g.add_tensor("out", list(dims), dtype, tm2.TT_VAR, None, *q(out_q))
    if out_quant is not None:
        g.tensors[y].scales, g.tensors[y].zero_points = [f32(out_q[0])] * out_quant, [int(out_q[1])] * out_quant
    g.output_nodes = [g.add_node("inorm", "InstanceNorm", [src, gi, bi][:inputs], [y], eps=f32(eps))]
    return g


def single(dims, seed, eps=1e-5, gamma=None, beta=None, in_q=IN_Q, out_q=OUT_Q, x=None):
    g_, b_ = stats(dims[1], seed + 1000, gamma, beta)
    g = node_graph(DT_UINT8, dims, g_, b_, eps, in_q, out_q)
    return g, lh.random_bytes(seed, DT_UINT8, dims) if x is None else np.ascontiguousarray(x, np.uint8).reshape(dims)


def order_sensitive_input(planes=6, hw=4099, seed=ORDER_SEED):
    """planes of `hw` bytes drawn from 236 .. 255: the region where the order of the two sums shows in the bytes"""
    return np.random.default_rng(seed).integers(236, 256, size=(1, planes, hw, 1)).astype(np.uint8)


def order_sensitive(planes=6, hw=4099, seed=ORDER_SEED):
    x = order_sensitive_input(planes, hw, seed)
    return single(x.shape, seed, 1e-5, 1.0, 0.0, ORDER_IN_Q, ORDER_OUT_Q, x)


def tiny_spread():
    """plane 0 constant (var 0: a = gamma / sqrt(eps), the double path alone), plane 1 constant but for one byte, plane 2 constant at
    byte 0, plane 3 two values"""
    x = np.full((1, 4, 5, 7), 131, np.uint8)
    x[0, 1, 2, 3] = 132
    x[0, 2] = 0
    x[0, 3, :, ::2] = 130
    return single(x.shape, 11, 1e-5, [1.0, 1.0, -0.75, 1.25], [0.25, 0.0, 0.1, -0.3], (0.02, 128), (0.05, 128), x)


def plane_bytes(x, table_of_plane):
    """the whole operator on an (N, C, H, W) array of bytes from the per-plane byte maps: table_of_plane(n, c, bytes) -> 256 bytes"""
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        for c in range(x.shape[1]):
            out[n, c] = table_of_plane(n, c, x[n, c].reshape(-1))[x[n, c]]
    return out


def _seq_sum(v):
    s = np.float32(0)
    for e in v:
        s = np.float32(s + e)
    return s


def _pair_sum(v):
    if len(v) <= 8:
        return _seq_sum(v)
    h = len(v) // 2
    return np.float32(_pair_sum(v[:h]) + _pair_sum(v[h:]))


def numpy_plane_map(bytes_, gamma, beta, eps, in_q, out_q, pairwise):
    """the restatement's operations in numpy, every fused multiply-add as a double product and sum rounded once to float: the 256-entry
    map of one plane with both sums sequential (pairwise False: tamd_instancenorm_plane's own order; the tests hold this function to
    it) or pairwise (True: a deliberately WRONG order, which lives here and not in the library)"""
    f, d = np.float32, np.float64
    dq = lambda u: (u.astype(np.float32) - f(in_q[1])) * f(in_q[0])
    v = dq(np.asarray(bytes_, np.uint8).reshape(-1))
    n, add = len(v), (_pair_sum if pairwise else _seq_sum)
    mean = f(add(v) / f(n))
    t = v - mean
    if pairwise:
        sq = add(t * t)
    else:
        body = n - n % 4
        sq = add(t[:body] * t[:body])
        for e in t[body:]:
            sq = f(d(e) * d(e) + d(sq))
    var = f(sq / f(n))
    a = f(d(f(gamma)) / np.sqrt(d(f(var + f(eps)))))
    b = f(d(-mean) * d(a) + d(f(beta)))
    y = (dq(np.arange(256, dtype=np.uint8)).astype(d) * d(a) + d(b)).astype(np.float32)
    r = (y / f(out_q[0]) + f(out_q[1])).astype(np.float32)
    r = np.where(r >= 0, np.floor(r.astype(d) + 0.5), np.ceil(r.astype(d) - 0.5))            # roundf: halves away from zero
    return np.clip(r, 0, 255).astype(np.uint8)


def numpy_statement(g, x, pairwise):
    """a one-node graph's output from numpy_plane_map"""
    node = g.nodes[g.output_nodes[0]]
    xt, yt = g.tensors[node.inputs[0]], g.tensors[node.outputs[0]]
    gamma, beta = (np.asarray(g.tensors[i].data, np.float32).reshape(-1) for i in node.inputs[1:3])
    return plane_bytes(x, lambda n, c, b: numpy_plane_map(b, gamma[c], beta[c], node.params["eps"], (xt.scales[0], xt.zero_points[0]),
                                                          (yt.scales[0], yt.zero_points[0]), pairwise))


def restatement(g, x):
    """a one-node graph's output from tamd_instancenorm_plane"""
    node = g.nodes[g.output_nodes[0]]
    xt, yt = g.tensors[node.inputs[0]], g.tensors[node.outputs[0]]
    gamma, beta = (np.asarray(g.tensors[i].data, np.float32).reshape(-1) for i in node.inputs[1:3])

    def table(n, c, bytes_):
        rc, tab, _ = capi.instancenorm_plane(bytes_, float(gamma[c]), float(beta[c]), node.params["eps"], xt.scales[0], xt.zero_points[0], yt.scales[0],
                                             yt.zero_points[0])
        assert rc == 0, rc
        return tab
    return plane_bytes(x, table)


class Gen(ih.Neck):
    """interp_helpers.Neck with the nodes of a generator block: InstanceNorm and the ReLU behind it"""

    def inorm(self, eps=1e-5, out_q=None, src=None, seed=7):
        x = self.cur if src is None else src
        d = self.dims(x)
        name = self._name("inorm")
        gamma, beta = stats(d[1], seed + self.k)
        ins = [x, self.g.add_const(name + "_gamma", gamma, DT_FP32), self.g.add_const(name + "_beta", beta, DT_FP32)]
        q = out_q if out_q is not None else (None if self.dtype == DT_FP32 else (4.0 / 255.0 * 2, 0 if self.dtype == DT_INT8 else 128))
        y = self._var(name, d, q)
        self.last = self.g.add_node(name, "InstanceNorm", ins, [y], eps=f32(eps))
        self.cur = y
        return y

    def relu(self, slope=0.0, out_q=None, src=None):
        x = self.cur if src is None else src
        name = self._name("relu")
        q = out_q if out_q is not None else (None if self.dtype == DT_FP32 else (self.scale(x) * 0.6, 0 if self.dtype == DT_INT8 else 9))
        y = self._var(name, self.dims(x), q)
        self.last = self.g.add_node(name, "ReLU", [x], [y], negative_slope=f32(slope))
        self.cur = y
        return y

    def done_with(self, outputs):
        g, x = self.done()
        g.output_nodes = list(outputs)
        return g, x


def generator_block(dtype, dims=(1, 8, 9, 7), cmid=12, cout=8, slope=0.0, seed=95):
    """conv3x3 -> InstanceNorm -> ReLU (slope > 0: leaky) -> conv3x3, the block of fast style transfer / CycleGAN / AnimeGAN generators"""
    k = Gen(seed, dtype, dims)
    k.conv(cmid, 3, 1)
    k.inorm()
    k.relu(slope)
    k.conv(cout, 3, 1)
    return k.done()


def relu_behind(dims=(2, 5, 5, 7), slope=0.0, seed=96):
    """data -> InstanceNorm -> ReLU: the ReLU is the only reader and the tensor between is no output, so it is composed into the map"""
    k = Gen(seed, DT_UINT8, dims, in_q=IN_Q)
    k.inorm(out_q=OUT_Q)
    k.relu(slope)
    return k.done()


def relu_not_alone(dims=(1, 3, 6, 6), seed=97):
    """data -> InstanceNorm -> ReLU with the InstanceNorm's output a graph output as well: the ReLU stays a launch of its own"""
    k = Gen(seed, DT_UINT8, dims, in_q=IN_Q)
    k.inorm(out_q=OUT_Q)
    mid = k.last
    k.relu(0.1)
    return k.done_with([mid, k.last])


def concat_and_second_reader(dims=(1, 3, 5, 7), seed=98):
    """y = InstanceNorm(data); Concat([conv(data), y]) at y's quantisation -> conv, and a ReLU that reads y too: the output owns its
    buffer (planes of 35 bytes, never aligned), the Concat copies"""
    k = Gen(seed, DT_UINT8, dims, in_q=IN_Q)
    data = k.cur
    y = k.inorm(out_q=OUT_Q, src=data)
    side = k.conv(2, 1, src=data)
    k.requant(side, OUT_Q)
    k.concat([side, y], OUT_Q)
    k.conv(4, 1)
    head = k.last
    k.relu(0.0, src=y)
    return k.done_with([head, k.last])


# the single-node cases: id -> (dims, kwargs of single()).  What each is for is in tests/test_gpu_instnorm.py
SINGLE = {}
for _n, _c in ((1, 1), (1, 3), (1, 4), (1, 5), (2, 65)):
    SINGLE["planes_%d" % (_n * _c)] = ((_n, _c, 3, 7), {})
for _hw in (1, 15, 16, 17, 1024, 1025, 4099):
    SINGLE["hw_%d" % _hw] = ((1, 3, _hw, 1) if _hw % 2 else (1, 3, _hw // 2, 2), {})
SINGLE["saturates_both_ends"] = ((1, 4, 6, 6), dict(gamma=[3.0, -3.0, 2.5, 4.0], beta=[0.0, 0.0, 1.5, -1.5], out_q=(0.01, 128)))
SINGLE["gamma_zero_eps_1"] = ((2, 3, 5, 5), dict(gamma=[0.0, 1.0, -40.0], beta=[0.7, -0.2, 0.0], eps=1.0))


def gpu_cases():
    """{id: builder}: every case the GPU tests run; a builder returns (graph, input)"""
    cases = {k: (lambda d=d, kw=kw: single(d, 5, **kw)) for k, (d, kw) in SINGLE.items()}
    cases["order_sensitive"] = order_sensitive
    cases["tiny_spread"] = tiny_spread
    cases["relu_folded"] = lambda: relu_behind(slope=0.0)
    cases["leaky_relu_folded"] = lambda: relu_behind(slope=0.1)
    cases["relu_not_alone"] = relu_not_alone
    cases["concat_and_second_reader"] = concat_and_second_reader
    cases["generator_block"] = lambda: generator_block(DT_UINT8)
    cases["generator_block_batch2"] = lambda: generator_block(DT_UINT8, dims=(2, 8, 9, 7))
    return cases


def reference_outputs(ref, g, x):
    return ref.run_model(tm2.write_tm2(g), x, ref.MODE_UINT8)


def golden():
    return np.load(GOLDEN)


def golden_entry(case, x, outs):
    """a case's seeded input and the reference's outputs"""
    e = {case + "__n": np.int32(len(outs)), case + "__in": x}
    for i, o in enumerate(outs):
        e["%s__out%d" % (case, i)] = o
    return e


def _desc(dtype, dims, ttype=1, quant=None, q=None, data=None, keep=None):
    d = lh.TensorDesc()
    d.dtype, d.ttype, d.dim_num = dtype, ttype, len(dims)
    d.quant_num = (0 if dtype == 0 else 1) if quant is None else quant
    for i, v in enumerate(dims):
        d.dims[i] = v
    if q is not None and d.quant_num == 1:
        s, z = (C.c_float * 1)(q[0]), (C.c_int * 1)(int(q[1]))
        keep.extend([s, z])
        d.scales, d.zero_points = C.cast(s, C.c_void_p), C.cast(z, C.c_void_p)
    if data is not None:
        a = np.ascontiguousarray(data)
        keep.append(a)
        d.data = a.ctypes.data_as(C.c_void_p)
    return d


def ask(dtype, dims, gamma=None, beta=None, eps=1e-5, const_input=False, in_quant=None, out_quant=None, with_param=True, inputs=3, in_q=IN_Q, out_q=OUT_Q,
        stat_dtype=0, stat_const=True, stat_elems=None, out_dims=None, values=True):
    """tamd_node_supported for an InstanceNorm node (dtype, stat_dtype: the C ABI's codes); values False: descriptors alone, as a caller
    without payloads asks"""
    c = dims[1] if len(dims) > 1 else 1
    gamma = np.ones(c, np.float32) if gamma is None else np.asarray(gamma, np.float32)
    beta = np.zeros(c, np.float32) if beta is None else np.asarray(beta, np.float32)
    p = capi.InstanceNormParam(eps)
    n = lh.NodeDesc()
    n.op, n.input_num, n.output_num = OP_INSTANCENORM, inputs, 1
    if with_param:
        n.param = C.cast(C.pointer(p), C.c_void_p)
    keep = []
    sd = [stat_elems if stat_elems is not None else c]
    st = lambda a: _desc(stat_dtype, sd, 2 if stat_const else 1, quant=0, data=a if values else None, keep=keep)
    outs = (lh.TensorDesc * 1)(_desc(dtype, dims if out_dims is None else out_dims, quant=out_quant, q=out_q if values else None, keep=keep))
    ins = (lh.TensorDesc * 3)(_desc(dtype, dims, 2 if const_input else 1, quant=in_quant, q=in_q if values else None, keep=keep), st(gamma), st(beta))
    return capi.lib().tamd_node_supported(C.byref(n), ins, inputs, outs, 1)


def library_outcome(tm_bytes):
    """(shape the library infers for output 0, the error prerun leaves): both are made before the device is touched"""
    L = capi.lib()
    h = L.tamd_graph_load_tm2(tm_bytes, len(tm_bytes))
    assert h, L.tamd_last_error()
    rc = L.tamd_graph_prerun(h, None)
    dims, dt = (C.c_int * 8)(), C.c_int()
    nd = L.tamd_graph_output_desc(h, 0, dims, C.byref(dt), None, None)
    err = L.tamd_last_error().decode() if rc != 0 else ""
    L.tamd_graph_destroy(h)
    return tuple(dims[k] for k in range(nd)), err
