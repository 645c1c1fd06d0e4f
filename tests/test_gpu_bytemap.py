"""Eltwise with a constant scalar and the unary Eltwise types on the device (csrc/lut_tables.cc: tamd_eltwise_table + misc_kernels.hip:
lut_u8): device bytes == the real reference library's bytes, from the committed golden (tests/golden/bytemap_cases.npz, always) and from
the reference itself (where oracle/_ref is built), through the C ABI with pooled tensors (the default) and with keep_tensors = 1, twice
per graph, and through the plugin.  Every node of these forms alone is exactly one lut_u8 launch, and every byte-pure chain (x *
sigmoid(x), the HardSwish decomposition, SUB_SCALAR -> PROD_SCALAR) is ONE, with TAMD_PIN=bytemap_chain=0 the launch list of the nodes
one by one and the same bytes.  The shapes are the smallest at which the launch can go wrong: the tensor that holds every byte once,
and (2, 5, 3, 3) -- 90 bytes: a ragged last vector; int8: 11 padding lanes per pixel, which must come out as zero although the tables
map byte 0 elsewhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bytemap_helpers as bh
import lut_helpers as lh
from oracle import ref_capi
from tengine_amd import tm2
from tengine_amd.tm2 import DT_INT8, DT_UINT8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = bh.gpu_cases()
KERNELS = ["lut_u8", "eltwise_i8", "eltwise_u8", "eltwise_relu_i8", "chan_lut_u8", "prelu_u8"]


@pytest.fixture(scope="module")
def golden():
    return bh.golden()


def _counts(names):
    return {k: names.count(k) for k in KERNELS if names.count(k)}


def _run_case(case, golden, expect, flat=False):
    """pooled and keep_tensors = 1 against the golden and, where it is built, the reference on the same bytes; expect: {kernel: count} of
    the byte-map and the same-shape Eltwise kernels in the launch list.  flat: compare element order alone (behind a FullyConnected the
    library's output is [N, C] where the reference keeps (N, C, 1, 1)).  Returns the outputs of the pooled run"""
    dtype, build = CASES[case]
    g, xs = build()
    for i, x in enumerate(xs):
        assert np.array_equal(golden["%s__in%d" % (case, i)], x)
    b = tm2.write_tm2(g)
    want = bh.reference_outputs(ref_capi, g, xs, dtype) if ref_capi.available() else None
    first = None
    for keep in (False, True):
        got, names, _ = bh.device_outputs(b, xs, keep_tensors=keep)
        assert _counts(names) == expect, names
        if flat:
            got = [o.reshape(golden["%s__out%d" % (case, i)].shape) for i, o in enumerate(got)]
        if want is not None:
            assert len(got) == len(want)
            for w, o in zip(want, got):
                assert w.shape == o.shape and w.dtype == o.dtype, (w.shape, o.shape)
                assert np.array_equal(w, o), (keep, int((w != o).sum()), w.size)
        assert bh.equals_golden(golden, case, got), (case, keep, [int((golden["%s__out%d" % (case, i)] != o).sum()) for i, o in enumerate(got)])
        first = first or got
    return first


@pytest.mark.parametrize("typ,dtype", bh.RUNNING_PAIRS, ids=["%s-%s" % (bh.NAME[t], bh.TAG[d]) for t, d in bh.RUNNING_PAIRS])
def test_every_running_pair_alone(typ, dtype, golden):
    """each (type, data type) pair as a one-node graph: on the tensor that holds all 256 bytes the output IS tamd_eltwise_table's bytes;
    on (2, 5, 3, 3) random bytes, a ragged end, and in int8 a channel padding 5 -> 16.  One lut_u8 launch each"""
    tag = "%s_%s" % (bh.TAG[dtype], bh.NAME[typ])
    got = _run_case("all_" + tag, golden, {"lut_u8": 1})[0]
    s = [s for s in bh.PARAM_SETS if s[1] == typ and s[2] == dtype and s[0].endswith("_1")][0]
    rc, tab = bh.table_of(*s[1:])
    assert rc == 0 and np.array_equal(got.reshape(-1).view(np.uint8), tab)
    rag = _run_case("ragged_" + tag, golden, {"lut_u8": 1})[0]
    _, xs = CASES["ragged_" + tag][1]()
    assert rag.shape == (2, 5, 3, 3) and np.array_equal(rag.view(np.uint8), tab[xs[0].view(np.uint8)])


def _child(case, pin, tmp_path):
    """the case in a fresh child process under TAMD_PIN=<pin> (the planners read it at prerun): (kernel counts, outputs)"""
    out = str(tmp_path / (case + ".npz"))
    code = "import sys; sys.path[:0] = [%r, %r]; import bytemap_helpers as bh; bh.child_main(%r, %r)" % (ROOT, os.path.join(ROOT, "tests"), case, out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TAMD_PIN=pin), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    return _counts([str(k) for k in z["names"]]), [z["out%d" % i] for i in range(len(z.files) - 1)]


# (case, the launches of the nodes one by one -- TAMD_PIN=bytemap_chain=0 --: {kernel: count})
CHAIN_CASES = [
    ("i8_silu", {"lut_u8": 1, "eltwise_i8": 1}), ("u8_silu", {"lut_u8": 1, "eltwise_u8": 1}),
    ("i8_hardswish", {"lut_u8": 3, "eltwise_i8": 1}), ("u8_hardswish", {"lut_u8": 3, "eltwise_u8": 1}), ("u8_hardswish_div", {"lut_u8": 3, "eltwise_u8": 1}),
    ("i8_normalise", {"lut_u8": 2}), ("u8_normalise", {"lut_u8": 2}),
    ("i8_unary_chain", {"lut_u8": 2}), ("u8_unary_chain", {"lut_u8": 2}),
    ("i8_two_branches", {"lut_u8": 2, "eltwise_i8": 1}), ("u8_two_branches", {"lut_u8": 2, "eltwise_u8": 1}),
]


@pytest.mark.parametrize("case,apart", CHAIN_CASES, ids=[c[0] for c in CHAIN_CASES])
def test_byte_pure_chain_is_one_launch(case, apart, golden, tmp_path):
    """conv -> SiLU -> conv on (2, 8, 5, 3); conv -> SUM 3 -> Clip(0, 6) -> PROD(x, .) -> PROD_SCALAR 1/6 (uint8 also DIV 6) -> conv on
    (1, 16, 7, 7); SUB_SCALAR -> PROD_SCALAR on the graph input (uint8: MobileFaceNet's fp32 constants 127.5 and 0.0078125), batch 2;
    SQUARE -> FLOOR between two convolutions; PROD(Clip(x), Sigmoid(x)), two table nodes on the source.  Each chain is ONE lut_u8 launch and nothing else of these kernels, the reference's bytes;
    a fresh child process with TAMD_PIN=bytemap_chain=0 runs the nodes one by one -- the launch list from before -- to the same bytes"""
    got = _run_case(case, golden, {"lut_u8": 1})
    counts, outs = _child(case, "bytemap_chain=0", tmp_path)
    assert counts == apart, counts
    assert len(outs) == len(got) and all(np.array_equal(a, b) for a, b in zip(outs, got))


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
def test_chain_guards(dtype, golden):
    """a Sigmoid whose tensor is a graph output too is written by its own launch, and the product reads it: no chain, both outputs the
    reference's.  A Clip with a second reader ends the set there: SUM 3 -> Clip as one launch, then the product and PROD_SCALAR by
    themselves"""
    tag = bh.TAG[dtype]
    got = _run_case(tag + "_silu_sigmoid_is_output", golden, {"lut_u8": 1, "eltwise_" + tag: 1})
    assert len(got) == 2
    got = _run_case(tag + "_hardswish_second_reader", golden, {"lut_u8": 2, "eltwise_" + tag: 1})
    assert len(got) == 2
    # Clip -> SQUARE is one launch although a Sigmoid of the same source, a graph output, lies between them in node order
    got = _run_case(tag + "_branch_beside_a_chain", golden, {"lut_u8": 2})
    assert len(got) == 2


@pytest.mark.parametrize("form,kernel", [(0, "chan_lut_u8"), (1, "prelu_u8")], ids=["chan_lut", "per_plane"])
@pytest.mark.parametrize("dims", bh.BN_SHAPES, ids=["x".join(map(str, d)) for d in bh.BN_SHAPES])
def test_batchnorm_forms_between_guards(dims, form, kernel, golden, monkeypatch):
    """chan_lut_u8 and prelu_u8's per-plane form, each pinned with TAMD_PIN=bn_form (read at prerun), on [3, 130] (C no multiple of 16:
    chunks straddle images), [2, 5, 7], (2, 5, 3, 3) (9-byte planes at odd offsets), (1, 3, 1, 17) and (1, 2, 8, 40) (planes of 320 bytes).
    The BatchNorm's output lies between two guard tensors written before it: all three are the reference's bytes, and the middle one
    is tamd_batchnorm_table's bytes of every channel"""
    monkeypatch.setenv("TAMD_PIN", "bn_form=%d" % form)
    case = "bn_" + "x".join(map(str, dims))
    got = _run_case(case, golden, {"lut_u8": 2, kernel: 1})
    k = bh.BN_SHAPES.index(dims)
    _, x, (st, iq, oq) = bh.bn_guarded_graph(dims, 30 + k)
    assert len(got) == 3 and np.array_equal(got[1], bh.bn_apply(bh.bn_tables(dims[1], iq, oq, st, 1.0, 2e-5, 0), x))


@pytest.mark.parametrize("dims,kernel", [((1, 2, 8, 40), "chan_lut_u8"), ((1, 2, 32, 40), "prelu_u8")], ids=["small_planes", "large_planes"])
def test_batchnorm_default_form(dims, kernel):
    """without a pin, planes below the threshold take chan_lut_u8 and planes of at least it the per-plane form; the same bytes"""
    g, x, (st, iq, oq) = bh.bn_guarded_graph(dims, 9)
    got, names, _ = bh.device_outputs(tm2.write_tm2(g), [x])
    assert _counts(names) == {"lut_u8": 2, kernel: 1}, names
    assert np.array_equal(got[1], bh.bn_apply(bh.bn_tables(dims[1], iq, oq, st, 1.0, 2e-5, 0), x))


@pytest.mark.parametrize("n", [1, 2])
def test_mobilefacenets_two_ends_as_one_graph(ref, n, golden):
    """SUB_SCALAR 127.5 -> PROD_SCALAR 0.0078125 -> conv 3x3 s2 -> PReLU -> bottleneck + SUM -> conv 1x1 -> PReLU -> depthwise 7x7 ->
    FullyConnected 128 -> BatchNorm on (N, 3, 14, 14): through the C ABI against the golden and the reference, then through create_graph /
    prerun / run_graph on device "HIP" -- one subgraph, the bytes of the CPU device, twice in a row"""
    import test_plugin_dropin as tp
    _run_case("u8_mobilefacenet_ends_b%d" % n, golden, {"lut_u8": 1, "eltwise_u8": 1, "prelu_u8": 4, "chan_lut_u8": 1}, flat=True)
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = bh.mobilefacenet_ends_graph(n)
    b = tm2.write_tm2(g)
    want = ref.run_model(b, x, ref.MODE_UINT8)
    rg = ref.RefGraph(b, ref.MODE_UINT8, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = [(dev, ops) for dev, _, r, ops in tp.placement(rg) if r]
    got = rg.outputs()
    rg.run()
    again = rg.outputs()
    rg.close()
    assert pl and pl[0][0] == "HIP", pl
    if built_here:
        assert len(pl) == 1, pl
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)


def test_int8_padding_lanes_stay_zero_in_front_of_a_convolution(golden):
    """conv1x1 (8 -> 5) -> SUM 0.7 -> conv3x3 pad 1 (5 -> 7) at (2, 8, 5, 3): the table maps byte 0 to a non-zero byte, and the second
    convolution reads the 11 lanes per pixel that lut_u8 must have written as zero"""
    _run_case("i8_padding", golden, {"lut_u8": 1})


@pytest.mark.parametrize("dtype", [DT_INT8, DT_UINT8], ids=["int8", "uint8"])
@pytest.mark.parametrize("build", [bh.normalise_graph, bh.hardswish_graph], ids=["normalise", "hardswish"])
def test_plugin_runs_the_graph_as_one_hip_subgraph(ref, build, dtype):
    """create_graph / prerun / run_graph (twice) of the reference library on device "HIP": the bytes of its CPU device, and the whole graph
    -- the scalar Eltwise nodes included -- in ONE "HIP" subgraph.  The placement is asserted when the plugin in use is the one this
    tree's build() compiled (tengine_amd/lib/); the copy under oracle/_ref/ travels with a prebuilt reference and may be older; the
    splitter itself is pinned in tests/test_bytemap_cpu.py"""
    import test_plugin_dropin as tp
    tp._load_plugin(ref)
    built_here = os.path.dirname(os.path.abspath(tp.PLUGIN)) == os.path.join(ROOT, "tengine_amd", "lib")
    g, x = build(dtype)
    b = tm2.write_tm2(g)
    mode = lh.ref_mode(ref, dtype)
    want = ref.run_model(b, x, mode)
    rg = ref.RefGraph(b, mode, 1, device="HIP", dev_opt=tp.HipOpt(b"HIP", C.sizeof(tp.HipOpt), 0, 1, 0))
    rg.set_input(x)
    rg.run()
    pl = tp.placement(rg)
    got = rg.outputs()
    rg.run()
    again = rg.outputs()
    rg.close()
    real = [(dev, ops) for dev, _, r, ops in pl if r]
    assert real and real[0][0] == "HIP", pl
    if built_here:
        assert len(real) == 1 and real[0][1].count("Eltwise") >= 2, (tp.PLUGIN, pl)
    assert len(want) == len(got) == len(again) >= 1
    for w, o, a in zip(want, got, again):
        assert np.array_equal(w, o) and np.array_equal(w, a)
