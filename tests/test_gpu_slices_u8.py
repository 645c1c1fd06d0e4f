"""uint8: each byte-exact convolution form writing a channel RANGE of a Concat's NCHW buffer (plan_nchw_buffers: out_img / out_c0; an
input that carries the Concat's scale and zero point is written in place and the Concat launches nothing).  Pinned with TAMD_PIN;
slice_helpers.u8_concat_graph puts three planes of a second convolution in front of, or behind, the form's own, so that its planes
start at an odd byte offset in one order.  Bytes against the oracle, exact."""
import numpy as np
import pytest

from helpers import pinned
from oracle import oracle
from slice_helpers import U8_CASES, U8_PATCH_NAMES, u8_case
from tengine_amd import capi, tm2

pytestmark = pytest.mark.gpu

SEEN = set()


@pytest.mark.parametrize("second", [True, False], ids=["behind_three_planes", "first"])
@pytest.mark.parametrize("case", sorted(U8_CASES))
def test_uint8_form_writes_its_range_of_the_concat(case, second):
    pins, cin, k, cout, tail, prefix = U8_CASES[case]
    g, x = u8_case(case, second)
    want = oracle.run_graph(g, x)[0]
    with pinned(**pins):
        gr = capi.Graph(tm2.write_tm2(g))
    gr.set_input(x)
    got = gr.run()[0].reshape(want.shape)
    prof = gr.profile(1)
    gr.close()
    names = [p["kernel"] for p in prof]
    mine = [p["kernel"] for p in prof if p["node"].split("+")[0] == "op"]
    assert len(mine) == 1 and mine[0].startswith(prefix), prof
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s (%s): %d of %d bytes differ, first at %s" % (case, mine[0], len(bad), want.size, bad[0].tolist())
    if tail == "pool":
        # a pooled tensor is not written in place (plan_u8's in_place: Convolution, ReLU, Upsample, Interp), so the pool fused into
        # the convolution's epilogue stores a dense tensor and the Concat copies it: one copy, for that input alone
        assert "+maxpool" in mine[0] and sum("concat" in kn for kn in names) == 1, prof
    else:
        assert not [kn for kn in names if "concat" in kn], prof
    if tail == "relu":
        assert "+relu" in mine[0], prof
    SEEN.add(mine[0].split("+")[0])


def test_census_every_patch_configuration_ran():
    """conv_u8_patch offers five configurations for 3x3 and 1x1 kernels: all ten wrote a Concat range above"""
    if not SEEN:                 # the cases above were deselected in this run
        for case in sorted(U8_CASES):
            test_uint8_form_writes_its_range_of_the_concat(case, True)
    assert set(U8_PATCH_NAMES.values()) <= SEEN, sorted(set(U8_PATCH_NAMES.values()) - SEEN)
    assert {"conv_u8_pw<k32>", "conv_u8_pw<k64>", "conv_u8_c3<c16>", "conv_u8_c3<c32>"} <= SEEN, sorted(SEEN)
    assert any(kn.startswith("conv_u8_rgb3x3") for kn in SEEN) and any(kn.startswith("conv_u8_mfma") for kn in SEEN), sorted(SEEN)
