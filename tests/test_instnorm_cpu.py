"""uint8 InstanceNorm on the device, the parts that need no GPU: the operator codes, the host restatement (tamd_instancenorm_plane)
against the real reference library on every byte, that the suite sees a wrong summation order, instancenorm_refusal's answers (each by its
name), the tmfile writer and both readers, where the plugin's splitter puts the node, the committed golden against the reference, the
planner's answer to "which form, and was the ReLU folded", and the restatement stand-alone under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import instnorm_helpers as nh
import lut_helpers as lh
import slice_op_helpers as so
from tengine_amd import capi, models, tm2
from tengine_amd.tm2 import DT_FP32, DT_INT8, DT_UINT8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, FP16, I8, U8 = 0, 1, 2, 3
HWS = (1, 2, 3, 15, 16, 17, 64, 255, 1024, 4099)
GAMMAS = {1: [-1.3], 3: [-1.3, 0.0, 40.0], 5: [-1.3, 0.0, 40.0, 1.0, -0.5]}
BETAS = {1: [0.4], 3: [0.4, -0.7, 0.05], 5: [0.4, -0.7, 0.05, 0.0, 2.0]}


def test_operator_codes():
    """fails without the feature: code 38 is nobody's"""
    L = capi.lib()
    assert nh.OP_INSTANCENORM == capi.OP_INSTANCENORM == 38
    assert [L.tamd_op_supported(38, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 1]
    assert [L.tamd_op_supported(37, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]
    assert [L.tamd_op_supported(39, dt) for dt in (F32, FP16, I8, U8)] == [0, 0, 0, 0]


def _grid():
    """every H * W with C, N and eps going round so that each value of each meets several sizes"""
    k = 0
    for hw in HWS:
        for c in (1, 3, 5):
            yield hw, c, (1, 2)[k % 2], (1e-5, 1e-3, 1.0)[(k // 2) % 3]
            k += 1


@pytest.mark.parametrize("pair", so.TABLE_SETS, ids=[s[0] for s in so.TABLE_SETS])
def test_restatement_is_the_reference_on_every_byte(ref, pair):
    """a one-node graph through the real reference against tamd_instancenorm_plane plane by plane: byte equality, over every plane size,
    C in {1, 3, 5}, N in {1, 2}, gamma negative, zero and large, beta non-zero, eps in {1e-5, 1e-3, 1}"""
    _, in_q, out_q = pair
    seen = set()
    for i, (hw, c, n, eps) in enumerate(_grid()):
        dims = (n, c, hw, 1) if hw % 2 or hw < 4 else (n, c, hw // 2, 2)
        g, x = nh.single(dims, 100 + i, eps, GAMMAS[c], BETAS[c], in_q, out_q)
        want = nh.reference_outputs(ref, g, x)[0]
        got = nh.restatement(g, x)
        assert want.shape == got.shape and np.array_equal(want, got), (dims, eps, int((want != got).sum()), want.size)
        seen.add((c, n, eps))
    assert {s[0] for s in seen} == {1, 3, 5} and {s[1] for s in seen} == {1, 2} and {s[2] for s in seen} == {1e-5, 1e-3, 1.0}


def test_restatement_returns_the_statistics_it_used():
    x = np.arange(1, 8, dtype=np.uint8)
    rc, tab, st = capi.instancenorm_plane(x, 2.0, 0.5, 1e-3, 0.5, 0, 0.25, 10)
    assert rc == 0 and tab.shape == (256,)
    v = x.astype(np.float32) * np.float32(0.5)
    assert st[0] == np.float32(14.0) and abs(float(st[1]) - float(((v - v.mean()) ** 2).sum())) < 1e-5
    a = 2.0 / np.sqrt(float(np.float32(st[1] / np.float32(7.0)) + np.float32(1e-3)))
    assert abs(float(st[2]) - a) < 1e-6 and abs(float(st[3]) - (0.5 - 2.0 * a)) < 1e-5
    assert capi.instancenorm_plane(np.zeros(0, np.uint8), 1.0, 0.0, 1e-5, 0.05, 0, 0.05, 0)[0] == -1          # an empty plane
    assert capi.instancenorm_plane(x, 1e30, 0.0, 1e-30, 1.0, 0, 1e-30, 0)[0] == -2                            # a value outside int


def test_the_suite_sees_a_wrong_summation_order(ref):
    """planes of 4099 bytes drawn from 236 .. 255 at (0.0173, 0), out (6 / 255, 128), gamma 1, beta 0, eps 1e-5, seed 3: large mean, small
    spread.  The reference's bytes equal the restatement's -- and those of its numpy statement with sequential sums -- and differ from
    those of the same numpy statement with pairwise sums.  Counted here against the real reference: 431 of 24 594 bytes differ."""
    g, x = nh.order_sensitive()
    want = nh.reference_outputs(ref, g, x)[0]
    assert np.array_equal(want, nh.restatement(g, x))
    assert np.array_equal(want, nh.numpy_statement(g, x, pairwise=False))      # the numpy statement is the restatement; only the order differs below
    wrong = nh.numpy_statement(g, x, pairwise=True)
    diff = int((want != wrong).sum())
    print("order_sensitive: %d of %d bytes differ under pairwise sums" % (diff, want.size))
    assert want.size == 24594 and diff >= 1


def _error(g):
    return nh.library_outcome(tm2.write_tm2(g))[1]


C3 = (np.ones(3, np.float32), np.zeros(3, np.float32))
X = (2, 3, 5, 7)
# (what, graph builder, the reason prerun names)
REFUSALS = [
    ("int8", lambda: nh.node_graph(DT_INT8, X, *C3, 1e-5, (0.05, 0), (0.03, 0)), "InstanceNorm does not run on the device in int8 graphs: the reference has no int8 kernel"),
    ("fp32", lambda: nh.node_graph(DT_FP32, X, *C3, 1e-5), "InstanceNorm runs on the device in uint8 graphs only"),
    ("empty_plane", lambda: nh.node_graph(DT_UINT8, (2, 3, 0, 7), *C3, 1e-5), "InstanceNorm: a plane is empty"),
    ("rank3", lambda: nh.node_graph(DT_UINT8, (3, 5, 7), np.ones(5, np.float32), np.zeros(5, np.float32), 1e-5), "InstanceNorm runs on the device on a 4-D tensor only"),
    ("const_x", lambda: nh.node_graph(DT_UINT8, X, *C3, 1e-5, data_const=True), "InstanceNorm: the data tensor must not be a constant"),
    ("gamma_len", lambda: nh.node_graph(DT_UINT8, X, np.ones(4, np.float32), np.zeros(4, np.float32), 1e-5), "InstanceNorm: gamma and beta must be fp32 constants of C elements"),
    ("gamma_type", lambda: nh.node_graph(DT_UINT8, X, *C3, 1e-5, stat_dtype=DT_UINT8), "InstanceNorm: gamma and beta must be fp32 constants of C elements"),
    ("gamma_kind", lambda: nh.node_graph(DT_UINT8, X, *C3, 1e-5, stat_const=False), "InstanceNorm: gamma and beta must be fp32 constants of C elements"),
    ("gamma_nan", lambda: nh.node_graph(DT_UINT8, X, np.array([1, np.nan, 1], np.float32), C3[1], 1e-5), "InstanceNorm: gamma and beta must be finite"),
    ("beta_inf", lambda: nh.node_graph(DT_UINT8, X, C3[0], np.array([0, 0, np.inf], np.float32), 1e-5), "InstanceNorm: gamma and beta must be finite"),
    ("eps_zero", lambda: nh.node_graph(DT_UINT8, X, *C3, 0.0), "InstanceNorm: eps must be finite and positive"),
    ("eps_negative", lambda: nh.node_graph(DT_UINT8, X, *C3, -1e-5), "InstanceNorm: eps must be finite and positive"),
    ("eps_nan", lambda: nh.node_graph(DT_UINT8, X, *C3, float("nan")), "InstanceNorm: eps must be finite and positive"),
    ("per_channel_in", lambda: nh.node_graph(DT_UINT8, X, *C3, 1e-5, in_quant=3), "InstanceNorm needs per-tensor quant params on both sides"),
    ("per_channel_out", lambda: nh.node_graph(DT_UINT8, X, *C3, 1e-5, out_quant=3), "InstanceNorm needs per-tensor quant params on both sides"),
    ("two_inputs", lambda: nh.node_graph(DT_UINT8, X, *C3, 1e-5, inputs=2), "InstanceNorm takes three inputs: the data, gamma and beta"),
    ("bound", lambda: nh.node_graph(DT_UINT8, X, np.full(3, 1e6, np.float32), C3[1], 1e-12, (1.0, 0), (1e-6, 0)),
     "InstanceNorm: a value could leave int before the reference's conversion (the bound on |y / out_scale + out_zp| reaches 2^30)"),
]


@pytest.mark.parametrize("what,build,reason", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_by_its_name(what, build, reason):
    """the file loads, and prerun names the reason before it touches the device"""
    err = _error(build())
    assert reason in err, (what, err)


def test_an_fp32_graph_and_an_empty_plane_are_refused_by_the_support_query():
    assert nh.ask(U8, X) == 1
    assert nh.ask(U8, X, values=False) == 1                                     # descriptors alone: the bound waits for prerun
    assert nh.ask(U8, (1, 1, 1, 1)) == 1 and nh.ask(U8, (7, 65, 1, 4099)) == 1  # any batch
    assert nh.ask(F32, X) == 0 and nh.ask(FP16, X) == 0 and nh.ask(I8, X, in_q=(0.05, 0), out_q=(0.03, 0)) == 0
    assert nh.ask(U8, (2, 3, 0, 7)) == 0 and nh.ask(U8, (2, 3, 5, 0)) == 0      # an empty plane
    assert nh.ask(U8, (3, 5, 7)) == 0 and nh.ask(U8, (1, 2, 3, 5, 7)) == 0
    assert nh.ask(U8, X, const_input=True) == 0 and nh.ask(U8, X, with_param=False) == 0 and nh.ask(U8, X, inputs=2) == 0
    assert nh.ask(U8, X, stat_elems=4) == 0 and nh.ask(U8, X, stat_dtype=U8) == 0 and nh.ask(U8, X, stat_const=False) == 0
    assert nh.ask(U8, X, gamma=[1, np.inf, 1]) == 0 and nh.ask(U8, X, beta=[np.nan, 0, 0]) == 0
    assert nh.ask(U8, X, eps=0.0) == 0 and nh.ask(U8, X, eps=-1.0) == 0 and nh.ask(U8, X, eps=float("inf")) == 0
    assert nh.ask(U8, X, in_quant=3) == 0 and nh.ask(U8, X, out_quant=0) == 0
    assert nh.ask(U8, X, out_dims=(2, 3, 5, 8)) == 0
    big = dict(gamma=[1e6] * 3, eps=1e-12, in_q=(1.0, 0), out_q=(1e-6, 0))
    assert nh.ask(U8, X, **big) == 0 and nh.ask(U8, X, values=False, **big) == 1


def test_the_bound_stands_where_the_issue_puts_it():
    """(255 * in_scale * max|gamma| / sqrt(eps) + max|beta|) / out_scale + |out_zp| below 2^30, on both sides of it"""
    f = lambda g: (255.0 * 1.0 * g / np.sqrt(float(np.float32(1e-4))) + 1.0) / float(np.float32(1e-3)) + 7
    lo, hi = 42.0, 42.2
    assert f(lo) < 2.0 ** 30 < f(hi)
    q = dict(eps=1e-4, in_q=(1.0, 0), out_q=(1e-3, 7), beta=[1.0, 0.0, -0.5])
    assert nh.ask(U8, X, gamma=[lo, 1.0, -3.0], **q) == 1 and nh.ask(U8, X, gamma=[1.0, -hi, 3.0], **q) == 0


def test_writer_and_both_readers_round_trip_operator_66(ref):
    """fails without the feature: the library's reader does not know tm2 operator 66 and the file cannot be loaded"""
    assert tm2.OPTYPE["InstanceNorm"] == 66
    g, x = nh.single((1, 3, 4, 5), 9, eps=0.0625)
    b = tm2.write_tm2(g)
    node = [n for n in tm2.read_tm2(b).nodes if n.op == "InstanceNorm"]
    assert len(node) == 1 and node[0].params == {"eps": 0.0625} and len(node[0].inputs) == 3
    assert capi.instancenorm_plan(b, g.output_nodes[0]) == (1, -1)              # the library's reader: a node the device runs
    # .. and it read eps = 0.0625 and no other value: the rule's bound is 255 * gamma / sqrt(eps) / 1e-3 here, 1.02e6 * gamma at 0.0625,
    # and 2^30 lies between gamma 1052 and 1054 for that eps alone (eps 0.0627 lets 1054 through, eps 0.0623 refuses 1052)
    def loads(gamma, eps):
        gg = nh.node_graph(DT_UINT8, (1, 1, 4, 5), [gamma], [0.0], eps, (1.0, 0), (1e-3, 0))
        return capi.instancenorm_plan(tm2.write_tm2(gg), gg.output_nodes[0]) is not None
    assert loads(1052.0, 0.0625) and not loads(1054.0, 0.0625)
    assert loads(1054.0, 0.0627) and not loads(1052.0, 0.0623)
    want = nh.reference_outputs(ref, g, x)[0]                                    # the reference's loader
    assert np.array_equal(want, nh.restatement(g, x))                            # .. with the same eps: 0.0625 against 1e-5 changes bytes
    g5, _ = nh.single((1, 3, 4, 5), 9, eps=1e-5)
    assert not np.array_equal(want, nh.restatement(g5, x))
    g.nodes[g.output_nodes[0]].params = {}                                       # the default is instancenorm.c's init_op
    assert abs([n for n in tm2.read_tm2(tm2.write_tm2(g)).nodes if n.op == "InstanceNorm"][0].params["eps"] - 1e-5) < 1e-12


def test_models_builder_writes_the_block():
    gf = models.generator_block_fp32(1, 8, 12)
    assert [n.op for n in gf.nodes if n.op not in ("Const", "InputOp")] == ["Convolution", "InstanceNorm", "ReLU", "Convolution"]
    gq = models.quantize_uint8(gf)
    n = [n for n in gq.nodes if n.op == "InstanceNorm"][0]
    assert [gq.tensors[i].dtype for i in n.inputs] == [DT_UINT8, DT_FP32, DT_FP32] and gq.tensors[n.outputs[0]].dims == [1, 8, 12, 12]
    assert capi.instancenorm_plan(tm2.write_tm2(gq), gq.nodes.index(n))[1] >= 0


def _real(pl):
    return [(dev, [o for o in ops if o not in ("InputOp", "Const")]) for dev, _, r, ops in pl if r]


def test_plugin_keeps_the_generator_block_in_one_hip_subgraph(ref):
    """fails without the feature: the plugin's operator table does not know the node and the split gives HIP / CPU / HIP"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = nh.generator_block(DT_UINT8)
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert len(real) == 1 and real[0][0] == "HIP" and real[0][1] == ["Convolution", nh.REF_OP_NAME, "ReLU", "Convolution"], real


@pytest.mark.parametrize("dtype", [DT_INT8, DT_FP32], ids=["int8", "fp32"])
def test_plugin_leaves_the_node_of_other_graph_types_to_the_cpu_device(ref, dtype):
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    g, x = nh.generator_block(dtype)
    real = _real(tp._split_only(ref, g, x, lh.ref_mode(ref, dtype)))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True], real
    assert real[1][1][0] == nh.REF_OP_NAME and "Convolution" in real[0][1] and "Convolution" in real[2][1], real


def test_plugin_leaves_a_refused_node_to_the_cpu_device(ref):
    """eps 0 is not the device's: the graph loads, and the node stays where the reference runs it, between two device subgraphs"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    k = nh.Gen(94, DT_UINT8, (1, 4, 6, 6))
    k.conv(4, 1)
    k.inorm(eps=0.0)
    k.conv(4, 1)
    g, x = k.done()
    real = _real(tp._split_only(ref, g, x, ref.MODE_UINT8))
    assert [dev == "HIP" for dev, _ in real] == [True, False, True] and real[1][1] == [nh.REF_OP_NAME], real


def test_the_planner_says_which_form_and_whether_the_relu_was_folded(monkeypatch):
    cases = nh.gpu_cases()

    def plan(case):
        g, _ = cases[case]()
        ni = [i for i, n in enumerate(g.nodes) if n.op == "InstanceNorm"][0]
        relu = [i for i, n in enumerate(g.nodes) if n.op == "ReLU" and n.inputs[0] == g.nodes[ni].outputs[0]]
        return capi.instancenorm_plan(tm2.write_tm2(g), ni), relu
    monkeypatch.delenv("TAMD_PIN", raising=False)
    for case in ("relu_folded", "leaky_relu_folded", "generator_block"):
        (form, rj), relu = plan(case)
        assert form == 1 and [rj] == relu, case                                  # small planes: one launch by default; the ReLU inside
    assert plan("relu_not_alone")[0] == (1, -1)                                  # the tensor between is a graph output
    assert plan("concat_and_second_reader")[0] == (1, -1)                        # two readers
    assert plan("planes_3")[0] == (1, -1)
    # the measured threshold (profiles/instnorm.txt): one launch up to 4096 bytes a plane, two launches above, whatever N * C is
    for dims, form in (((1, 2, 64, 64), 1), ((3, 2, 4096, 1), 1), ((1, 2, 4097, 1), 0), ((1, 1, 128, 128), 0), ((4, 7, 1, 1), 1)):
        g = nh.node_graph(DT_UINT8, dims, np.ones(dims[1], np.float32), np.zeros(dims[1], np.float32), 1e-5)
        assert capi.instancenorm_plan(tm2.write_tm2(g), g.output_nodes[0]) == (form, -1), dims
    assert plan("hw_4099")[0] == (0, -1) and plan("hw_1025")[0] == (1, -1)
    monkeypatch.setenv("TAMD_PIN", "instnorm_form=0")
    assert plan("relu_folded")[0][0] == 0 and plan("relu_folded")[0][1] >= 0
    monkeypatch.setenv("TAMD_PIN", "instnorm_form=1")
    assert plan("hw_4099")[0] == (1, -1)
    monkeypatch.setenv("TAMD_PIN", "instnorm_relu=0")
    assert plan("relu_folded")[0] == (1, -1)
    g, _ = cases["relu_folded"]()
    assert capi.instancenorm_plan(tm2.write_tm2(g), 0) is None                   # node 0 is the input


def test_golden_holds_every_case():
    z = nh.golden()
    cases = nh.gpu_cases()
    assert {k[:-3] for k in z.files if k.endswith("__n")} == set(cases)
    assert os.path.getsize(nh.GOLDEN) < 128 * 1024
    for case in nh.SINGLE:
        g, x = cases[case]()
        assert np.array_equal(z[case + "__in"], x) and int(z[case + "__n"]) == 1
        assert np.array_equal(z[case + "__out0"], nh.restatement(g, x)), case


def test_cases_hold_what_they_are_named_for():
    cases = nh.gpu_cases()
    z = nh.golden()
    assert set(nh.SINGLE) < set(cases) and len(cases) == len(nh.SINGLE) + 8 and len(nh.SINGLE) == 14
    planes = sorted(d[0] * d[1] for k, (d, _) in nh.SINGLE.items() if k.startswith("planes_"))
    assert planes == [1, 3, 4, 5, 130] and nh.SINGLE["planes_130"][0][:2] == (2, 65)
    assert sorted(d[2] * d[3] for k, (d, _) in nh.SINGLE.items() if k.startswith("hw_")) == [1, 15, 16, 17, 1024, 1025, 4099]
    assert all(d[1] == 3 for k, (d, _) in nh.SINGLE.items() if k.startswith("hw_"))          # planes 1, 2 start at odd addresses when H * W is odd
    sat = z["saturates_both_ends__out0"]
    assert (sat == 0).sum() > 4 and (sat == 255).sum() > 4
    g, x = cases["tiny_spread"]()
    assert len(np.unique(x[0, 0])) == 1 and (x[0, 1] != 131).sum() == 1 and len(np.unique(x[0, 3])) == 2
    out = z["tiny_spread__out0"]
    assert len(np.unique(out[0, 0])) == 1 and len(np.unique(out[0, 1])) == 2
    g, x = cases["order_sensitive"]()
    assert x.min() >= 236 and x.shape == (1, 6, 4099, 1)
    assert not np.array_equal(z["order_sensitive__out0"], nh.numpy_statement(g, x, pairwise=True))     # the golden sees a wrong order too
    for case, slope in (("relu_folded", 0.0), ("leaky_relu_folded", lh.f32(0.1))):
        g, _ = cases[case]()
        assert [n.params["negative_slope"] for n in g.nodes if n.op == "ReLU"] == [slope]
    g, _ = cases["concat_and_second_reader"]()
    y = [n for n in g.nodes if n.op == "InstanceNorm"][0].outputs[0]
    readers = [n.op for n in g.nodes if y in n.inputs]
    assert sorted(readers) == ["Concat", "ReLU"] and (5 * 7) % 16 != 0
    assert cases["generator_block_batch2"]()[1].shape[0] == 2


@pytest.mark.parametrize("case", sorted(nh.gpu_cases()))
def test_golden_is_the_real_reference(ref, case):
    """tests/golden/instnorm_cases.npz (tools/make_golden_instnorm.py) holds what the reference computes here"""
    z = nh.golden()
    g, x = nh.gpu_cases()[case]()
    assert np.array_equal(z[case + "__in"], x)
    want = nh.reference_outputs(ref, g, x)
    assert nh.equals_golden(z, case, want), case
    want[0].reshape(-1)[0] ^= 1                          # .. and the comparison is one: a single changed bit is seen
    assert not nh.equals_golden(z, case, want), case


PLANES = [  # size lo hi seed gamma beta eps in_scale in_zp out_scale out_zp
    (1, 0, 255, 1, 1.0, 0.0, 1e-5, 0.05, 77, 0.031, 12),
    (3, 0, 255, 2, -1.3, 0.4, 1e-3, 0.05, 0, 0.04, 255),
    (17, 0, 255, 3, 40.0, -0.7, 1.0, 0.0173, 101, 0.0291, 37),
    (1024, 0, 255, 4, 1.0, 0.0, 1e-5, 0.5, 3, 1.0, 4),
    (4099, 236, 255, 5, 1.0, 0.0, 1e-5, 0.0173, 0, 6.0 / 255.0, 128),
    (4098, 236, 255, 5, 1.0, 0.0, 1e-5, 0.0173, 0, 6.0 / 255.0, 128),
    (7, 131, 131, 6, 1.0, 0.25, 1e-5, 0.02, 128, 0.05, 128),
    (0, 0, 255, 7, 1.0, 0.0, 1e-5, 0.05, 77, 0.031, 12),
    (9, 0, 255, 8, 1e30, 0.0, 1e-30, 1.0, 0, 1e-30, 0),
]


def _plane(size, lo, hi, seed):
    s = (seed * 2654435761 + 12345) & 0xffffffff
    out = np.zeros(size, np.uint8)
    for j in range(size):
        s = (s * 1664525 + 1013904223) & 0xffffffff
        out[j] = lo + ((s >> 8) % (hi - lo + 1))
    return out


def test_the_restatement_runs_clean_under_the_sanitizers(tmp_path):
    """instnorm_check.cc + instnorm_tables.cc and nothing else, as a stand-alone host program (its own main) under the address and
    undefined-behaviour sanitizers: no report, and every line is what the library answers for the same plane"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "instnorm_check")
    csrc = os.path.join(ROOT, "tengine_amd", "csrc")
    subprocess.check_call([hipcc, "-std=c++17", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-I", csrc, os.path.join(ROOT, "tests", "csrc", "instnorm_check.cc"), os.path.join(csrc, "instnorm_tables.cc"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    lines = "\n".join(" ".join(repr(float(np.float32(v))) if isinstance(v, float) else str(v) for v in p) for p in PLANES) + "\n"
    out = subprocess.run([exe], input=lines, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(PLANES), out.stdout
    rcs = []
    for p, line in zip(PLANES, got):
        size, lo, hi, seed, gamma, beta, eps, isc, izp, osc, ozp = p
        f = line.split()
        rc, tab, st = capi.instancenorm_plane(_plane(size, lo, hi, seed), lh.f32(gamma), lh.f32(beta), lh.f32(eps), lh.f32(isc), izp, lh.f32(osc), ozp)
        assert int(f[0]) == rc, (p, line)
        rcs.append(rc)
        if rc == 0:
            h = 2166136261
            for b in tab:
                h = ((h ^ int(b)) * 16777619) & 0xffffffff
            assert [int(v, 16) for v in f[1:5]] == [int(v) for v in st.view(np.uint32)] and int(f[5], 16) == h, (p, line)
    assert rcs == [0, 0, 0, 0, 0, 0, 0, -1, -2]
    assert got[4] != got[5]                                                      # one element fewer: other statistics
