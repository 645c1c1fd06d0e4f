"""The int8 launchers beside the GEMM family with a channel slice on the side they read, the side they write, or both (see
slice_helpers.py): each depthwise 3x3 form, conv_direct_i8, the first-layer kernels, pool_i8 in its windowed and global forms,
FullyConnected into a 2-D Concat, and the two half-batch graphs of split_batch.  Bytes against the oracle, exact.

The byte -128: the reference's Concat of several inputs stores 127 for it even between equal scales, so a producer that writes into the
Concat's buffer has to -- Upsample (whose byte routine can emit 0x80), max-pool and nearest Interp, against the real reference."""
import functools

import numpy as np
import pytest

from helpers import pinned
from oracle import oracle
from slice_helpers import (FIRST_CASES, FUSER_CASES, GEMM_SHAPES, MINUS128_CASES, OP_CASES, block_concat_graph, chain_stem_graph, dw_case, fuser_case, fc_concat_graph, first_case, minus128_copies, minus128_graph, op_case,
                           slice_graph)
from tengine_amd import capi, tm2

pytestmark = pytest.mark.gpu

ORDERS = pytest.mark.parametrize("run_last", [True, False], ids=["op_last", "op_first"])


def device(g, x, inputs=1, **kw):
    gr = capi.Graph(tm2.write_tm2(g), **kw)
    for i in range(inputs):
        gr.set_input(x, i)
    got = gr.run()
    prof = gr.profile(1)
    gr.close()
    return got, prof


def kernels_of(prof, node="op"):
    """the launches of the node under test (a fused launch names its nodes joined by '+', the first one first)"""
    return [k["kernel"] for k in prof if k["node"].split("+")[0] == node]


def same(got, want, what):
    assert len(got) == len(want)
    for i, (o, w) in enumerate(zip(got, want)):
        o = o.reshape(w.shape)
        bad = np.argwhere(o != w)
        assert len(bad) == 0, "%s: output %d, %d of %d bytes differ, first at %s: got %d, want %d" % (
            what, i, len(bad), w.size, bad[0].tolist(), o[tuple(bad[0])], w[tuple(bad[0])])


def sliced(prof):
    """no copy at a Concat: its inputs were written in place, so the slices were in effect"""
    assert [k["kernel"] for k in prof].count("concat_copy_i8") == 0, prof


# ---- depthwise 3x3: every form ---------------------------------------------------------------------------------------------------
DW_SEEN = set()
DW_FORMS = [11, 12, 14, 21, 22]


def dw_name(form, stride):
    nf, th = divmod(form, 10)
    return "dwconv3x3_i8<%d,%d%s>" % (stride, nf, "" if th == 1 else ",r%d" % th)


@ORDERS
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("form", DW_FORMS)
def test_depthwise_3x3_form_on_slices(form, stride, run_last):
    g, x = dw_case(stride, run_last)
    with pinned(dw_form=form):
        got, prof = device(g, x)
    sliced(prof)
    assert kernels_of(prof) == [dw_name(form, stride)], prof
    same(got, oracle.run_graph(g, x), dw_name(form, stride))
    DW_SEEN.add((kernels_of(prof)[0], run_last))


def test_census_every_depthwise_form_ran_on_slices():
    for form in DW_FORMS:
        for stride in (1, 2):
            for run_last in (True, False):
                if (dw_name(form, stride), run_last) not in DW_SEEN:
                    test_depthwise_3x3_form_on_slices(form, stride, run_last)          # (deselected in this run)
    assert len({k for k, _ in DW_SEEN}) == 10 and len(DW_SEEN) == 20, sorted(DW_SEEN)


# ---- conv_direct_i8, pool_i8 (windowed and global) ------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("case", sorted(OP_CASES))
def test_direct_convolution_and_pooling_on_slices(case, run_last):
    g, x = op_case(case, run_last)
    got, prof = device(g, x)
    sliced(prof)
    assert kernels_of(prof) == [OP_CASES[case][5]], prof
    same(got, oracle.run_graph(g, x), case)


# ---- the first layer: its output a view ------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("case", sorted(FIRST_CASES))
def test_first_layer_kernels_write_a_slice(case, run_last):
    g, x, inputs = first_case(case, run_last)
    got, prof = device(g, x, inputs)
    sliced(prof)
    name = FIRST_CASES[case][8]
    assert kernels_of(prof) == [name] and [k["kernel"] for k in prof] == [name] * inputs, prof
    same(got, oracle.run_graph(g, x), case)


# ---- FullyConnected into a 2-D Concat --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_first", [False, True])
def test_two_fully_connected_write_one_concat_in_place(second_first):
    g, x = fc_concat_graph(7700, second_first)
    got, prof = device(g, x)
    assert len(prof) == 2 and {k["node"] for k in prof} == {"fc0", "fc1"}, prof
    same(got, oracle.run_graph(g, x), "fc")


# ---- two half-batch graphs -------------------------------------------------------------------------------------------------------
def test_split_batch_halves_address_the_same_slices():
    h, w, op, ins, outs = GEMM_SHAPES["pw_many"]
    g, x = slice_graph(7800, 4, h, w, op, ins, outs)
    want = oracle.run_graph(g, x)
    b = tm2.write_tm2(g)
    outs_by = {}
    for sb in (0, 2):
        gr = capi.Graph(b, split_batch=sb)
        assert gr.halves() == sb
        gr.set_input(x)
        outs_by[sb] = gr.run()
        gr.close()
        same(outs_by[sb], want, "split_batch=%d" % sb)
    assert not np.array_equal(want[1][:2], want[1][2:])


# ---- the byte -128 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def minus128(case):
    g, x = minus128_graph(case)
    return tm2.write_tm2(g), g, x


@pytest.mark.parametrize("case", sorted(MINUS128_CASES))
def test_minus_128_written_in_place_is_what_the_concat_would_store(ref, case):
    """Before UpsampleI8Args::fix128 every Upsample case failed here with `got -128, want 127` at the bytes the Upsample's byte routine
    yields as 0x80 (first: upsample_copy, (n, c, y, x) = (0, 14, 4, 4); upsample_map, (0, 1, 6, 2)); max-pool and nearest Interp
    saturate at -127 and passed.  Where the Upsample's tensor has a reader of its own, that reader needs the -128 the Concat's readers
    must not see: such an Upsample keeps its buffer and the Concat copies (slice_helpers.minus128_copies)"""
    b, g, x = minus128(case)
    want = ref.run_model(b, x, ref.MODE_INT8, 1)
    got, prof = device(g, x)
    names = [k["kernel"] for k in prof]
    assert names.count("concat_copy_i8") == minus128_copies(case) and len(kernels_of(prof)) == 1, prof
    same(got, want, "%s (%s)" % (case, kernels_of(prof)[0]))


# ---- fusers next to slices -------------------------------------------------------------------------------------------------------
# Each fuser has guards on views (graph_plan.hip / graph_plan_pairs.hip: find_pwdw_tail's `y.is_view`, try_dwpw's `dy.is_view`,
# dwpw_applicable's `& 15` tests, find_chain4's `y1.is_view`, try_block's sole_conv_behind).  The launch list asserted here is what
# those guards give for the graph: a change of a guard shows as another list; the bytes are the oracle's either way.
def fused_device(g, x, env, monkeypatch, inputs=1):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return device(g, x, inputs)


@ORDERS
@pytest.mark.parametrize("case", sorted(FUSER_CASES))
def test_pair_fusers_with_slices_on_their_outer_sides(case, run_last, monkeypatch):
    g, x = fuser_case(case, run_last)
    want = oracle.run_graph(g, x)
    env, name = FUSER_CASES[case][5], FUSER_CASES[case][6]
    got, prof = fused_device(g, x, env, monkeypatch)
    sliced(prof)
    mine = [k for k in prof if k["node"].split("+")[0] == "op"]
    assert len(mine) == 1 and mine[0]["node"] == "op+op1" and mine[0]["kernel"].startswith(name), prof
    same(got, want, case)
    # switched off, the two launches address the same slices
    got0, prof0 = fused_device(g, x, {k: "0" for k in env}, monkeypatch)
    sliced(prof0)
    assert [k["node"] for k in prof0 if k["node"].startswith("op")] == ["op", "op1"], prof0
    same(got0, want, case + " unfused")


@ORDERS
def test_chain_of_four_stem_whose_last_output_is_a_view(run_last, monkeypatch):
    g, x = chain_stem_graph(8100, run_last)
    want = oracle.run_graph(g, x)
    monkeypatch.setenv("TAMD_PIN", "chain4=2")
    got, prof = fused_device(g, x, {"TAMD_FUSE_PWDW": "2"}, monkeypatch, inputs=3)
    sliced(prof)
    assert len(prof) == 3 and all(k["kernel"].startswith("firstchain4_i8") for k in prof), prof
    assert [k["node"] for k in prof if k["node"].startswith("op")] == ["op+op1+op2+op3"], prof
    same(got, want, "chain4 stem")
    monkeypatch.setenv("TAMD_PIN", "chain4=0")
    got0, prof0 = fused_device(g, x, {"TAMD_FUSE_PWDW": "2"}, monkeypatch, inputs=3)
    sliced(prof0)
    assert len(prof0) == 6 and not any("chain4" in k["kernel"] for k in prof0), prof0
    same(got0, want, "chain4 stem as pairs")


def test_identity_block_in_front_of_a_concat(monkeypatch):
    g, x = block_concat_graph(8200)
    want = oracle.run_graph(g, x)
    got, prof = fused_device(g, x, {"TAMD_FUSE_BLOCK": "1"}, monkeypatch)
    names = [k["kernel"] for k in prof]
    # the leading convolution, the block as one launch, the side convolution (in place), one copy for the ReLU's output
    assert names.count("block_i8") == 1 and names.count("concat_copy_i8") == 1 and len(names) == 4, prof
    same(got, want, "block")
