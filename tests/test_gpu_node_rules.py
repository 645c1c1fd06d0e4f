"""The node-local rules that tamd_node_supported shares with the planners (tengine_amd/csrc/node_rules.h), at their boundaries on the
device: where the query says 1 the graph pre-runs and equals the oracle byte for byte; where it says 0 pre-run is refused on the host
with a message that names the node -- the planner and the query cannot drift apart."""
import numpy as np
import pytest

from helpers import conv_graph, i8_unary_graph, node_supported, u8_fc_graph
from oracle import oracle
from tengine_amd import capi, tm2

pytestmark = pytest.mark.gpu

CASES = {
    # uint8 FC keeps its input row in LDS as floats: 4 * hidden <= 60000
    "u8_fc_hidden_15000": (lambda: u8_fc_graph(7, 1, (15000,), 4), 1),
    "u8_fc_hidden_15001": (lambda: u8_fc_graph(7, 1, (15001,), 4), 0),
    # int8 softmax keeps the axis' exponentials in LDS: at most 16000 values
    "i8_softmax_16000": (lambda: i8_unary_graph(8, "Softmax", [1, 16000], out_scale=1e-4, axis=1), 1),
    "i8_softmax_16001": (lambda: i8_unary_graph(8, "Softmax", [1, 16001], out_scale=1e-4, axis=1), 0),
    # int8 implicit GEMM: a tap table of 128 entries (cin 16 on a 16 x 24 map)
    "i8_conv_8x16_taps_128": (lambda: conv_graph(9, 1, 16, 16, 24, 8, 8, kw=16), 1),
    "i8_conv_11x12_taps_132": (lambda: conv_graph(9, 1, 16, 16, 24, 8, 11, kw=12), 0),
}


@pytest.mark.parametrize("case", list(CASES))
def test_query_and_planner_agree_at_the_boundary(case):
    build, want_ok = CASES[case]
    g, x = build()
    assert node_supported(g) == want_ok
    blob = tm2.write_tm2(g)
    if not want_ok:
        with pytest.raises(capi.TamdError) as e:          # an error return of prerun: no launch list exists, nothing runs
            capi.Graph(blob)
        assert g.nodes[-1].name in str(e.value), str(e.value)
        return
    want = oracle.run_graph(g, x)[0]
    gr = capi.Graph(blob)
    gr.set_input(x)
    got = gr.run()[0].reshape(want.shape)
    gr.close()
    assert np.array_equal(want, got)
