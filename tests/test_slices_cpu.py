"""The conditions on the INPUTS of the slice tests (tests/test_gpu_slices_*.py), checked with the oracle where no GPU is needed: a
comparison of bytes proves something only where the expected bytes are varied (more than 20 distinct values), not saturated (fewer
than 5 % equal +-127), where the parts of the buffer a launch could read by mistake differ from the one it should read, and -- for the
-128 cases -- where the byte in question really is produced."""
import numpy as np
import pytest

import slice_helpers as sh
from oracle import oracle


def varied(outs, what):
    for i, o in enumerate(outs):
        distinct, sat = len(np.unique(o)), float(np.mean(np.abs(o.astype(np.int32)) == 127))
        assert distinct > 20 and sat < 0.05, "%s output %d: %d distinct bytes, %.1f %% at +-127" % (what, i, distinct, 100 * sat)


def parts_differ(mid, in_slice, what):
    """no two parts of mid of equal width hold the same bytes, and the operator's part is not a shifted copy of its neighbour"""
    widths, _ = sh.split_widths(in_slice)
    edges = np.cumsum([0] + widths)
    parts = [mid[:, a:b] for a, b in zip(edges[:-1], edges[1:])]
    for i in range(len(parts)):
        for j in range(i + 1, len(parts)):
            c = min(widths[i], widths[j])
            assert not np.array_equal(parts[i][:, :c], parts[j][:, :c]), what
            assert np.mean(parts[i][:, :c] != parts[j][:, :c]) > 0.9, what


ORDERS = pytest.mark.parametrize("run_last", [True, False], ids=["op_last", "op_first"])


@ORDERS
@pytest.mark.parametrize("shape", sorted(sh.GEMM_SHAPES))
def test_gemm_slice_cases(shape, run_last):
    g, x = sh.gemm_case(shape, run_last)
    outs = oracle.run_graph(g, x)
    varied(outs, shape)
    parts_differ(outs[0], sh.GEMM_SHAPES[shape][3], shape)
    # the launch order is the node order: the operator behind its output neighbours, or in front of them
    names = [n.name for n in g.nodes]
    assert all((names.index("op") > names.index(nb)) == run_last for nb in names if nb.startswith("nb"))


@pytest.mark.parametrize("shape", ["pw_many", "k3", "big"])
def test_gemm_eltwise_tail_cases(shape):
    g, x = sh.gemm_eltwise_case(shape)
    outs = oracle.run_graph(g, x)
    varied(outs, shape)
    parts_differ(outs[0], sh.GEMM_SHAPES[shape][3], shape)
    assert np.mean(outs[1] == 0) < 0.7          # the ReLU leaves enough of the sum


@ORDERS
@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_cases(stride, run_last):
    g, x = sh.dw_case(stride, run_last)
    outs = oracle.run_graph(g, x)
    varied(outs, "dw stride %d" % stride)
    parts_differ(outs[0], sh.OPS_IN, "dw")


@ORDERS
@pytest.mark.parametrize("case", sorted(sh.OP_CASES))
def test_direct_and_pool_cases(case, run_last):
    g, x = sh.op_case(case, run_last)
    outs = oracle.run_graph(g, x)
    varied(outs, case)
    parts_differ(outs[0], sh.OP_CASES[case][3], case)


@ORDERS
@pytest.mark.parametrize("case", sorted(sh.FIRST_CASES))
def test_first_layer_cases(case, run_last):
    g, x, inputs = sh.first_case(case, run_last)
    outs = oracle.run_graph(g, x)
    varied(outs, case)
    assert inputs == 3 and not np.array_equal(outs[0][:, 0:16], outs[0][:, 16:32]) and not np.array_equal(outs[0][:, 16:32], outs[0][:, 32:48])
    # both orders hold the same three stems
    assert sorted(n.name for n in g.nodes if n.op == "Convolution") == ["nb0", "nb2", "op"]


@pytest.mark.parametrize("second_first", [False, True])
def test_fc_case(second_first):
    g, x = sh.fc_concat_graph(7700, second_first)
    outs = oracle.run_graph(g, x)
    varied(outs, "fc")
    assert outs[0].shape == (3, 80)


def test_split_batch_case():
    h, w, op, ins, outs_ = sh.GEMM_SHAPES["pw_many"]
    g, x = sh.slice_graph(7800, 4, h, w, op, ins, outs_)
    outs = oracle.run_graph(g, x)
    varied(outs, "split batch")
    assert not np.array_equal(outs[1][:2], outs[1][2:])


@pytest.mark.parametrize("case", sorted(sh.MINUS128_CASES))
def test_minus_128_cases_hold_the_byte(case):
    """the Upsample cases: the restated byte map puts at least 8 bytes 0x80 into the slice that is written in place -- 4 where one image
    of 256 distinct byte values is copied (one -128, x2 in both directions: 4 is all that input can give); max-pool: whole windows of
    -128; nearest Interp: -128 in the input"""
    producer, s_in, n, first, side, _ = sh.MINUS128_CASES[case]
    g, x = sh.minus128_graph(case)
    assert len(np.unique(x)) == 256
    if producer == "upsample":
        up = sh.upsample_bytes(x, s_in, sh.CAT_SCALE)
        assert up.shape == (n, 16, 8, 8)
        floor = 4 if (n == 1 and s_in == sh.CAT_SCALE) else 8
        assert np.count_nonzero(up == -128) >= floor, np.count_nonzero(up == -128)
        assert len(np.unique(up)) > 20
    elif producer == "pool":
        win = x.reshape(n, 16, 8, 2, 8, 2).max(axis=(3, 5))
        assert np.count_nonzero(win == -128) >= 8
    else:
        assert np.count_nonzero(x == -128) >= 1


def test_minus_128_cases_against_the_reference(ref):
    """what the gap was: the reference stores 127 wherever the Upsample's byte routine yields 0x80, and nowhere -128"""
    from tengine_amd import tm2
    for case in sorted(sh.MINUS128_CASES):
        producer, s_in, n, first, side, _ = sh.MINUS128_CASES[case]
        g, x = sh.minus128_graph(case)
        want = ref.run_model(tm2.write_tm2(g), x, ref.MODE_INT8, 1)[0]
        mine = want[:, :16] if first else want[:, side:]
        assert not (want == -128).any(), case
        if producer == "upsample":
            up = sh.upsample_bytes(x, s_in, sh.CAT_SCALE)
            assert np.array_equal(np.where(up == -128, 127, up), mine), case


@pytest.mark.parametrize("second", [True, False])
@pytest.mark.parametrize("case", sorted(sh.U8_CASES))
def test_uint8_concat_range_cases(case, second):
    g, x = sh.u8_case(case, second)
    out = oracle.run_graph(g, x)[0]
    assert len(np.unique(out)) > 20 and np.mean((out == 0) | (out == 255)) < 0.05, case
    c0 = 3 if second else 0
    cout = sh.U8_CASES[case][3]
    assert out.shape[1] == 3 + cout and len(np.unique(out[:, c0:c0 + cout])) > 20
    if second and sh.U8_CASES[case][4] != "pool":
        assert (3 * out.shape[2] * out.shape[3]) % 2 == 1          # the operator's planes start at an odd byte offset


@ORDERS
@pytest.mark.parametrize("case", sorted(sh.FUSER_CASES))
def test_fuser_cases(case, run_last):
    g, x = sh.fuser_case(case, run_last)
    outs = oracle.run_graph(g, x)
    varied(outs, case)
    parts_differ(outs[0], sh.FUSER_CASES[case][3], case)


@ORDERS
def test_chain_stem_and_block_cases(run_last):
    for g, x in (sh.chain_stem_graph(8100, run_last), sh.block_concat_graph(8200)):
        outs = oracle.run_graph(g, x)
        varied(outs, g.name)
        assert np.mean(outs[0] == 0) < 0.7
