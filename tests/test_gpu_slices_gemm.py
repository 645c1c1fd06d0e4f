"""Every member of the int8 GEMM family with its input, its output, or both a channel SLICE of a wider buffer: what the planner hands
it wherever it removes a channel Concat (x = dptr + c_off with cs_in > cin; ldc > cout, c_off != 0, c_limit from store_limit).  The
race picks a member by speed alone, so each is pinned with TAMD_FORCE_GEMM on the shapes of slice_helpers.GEMM_SHAPES, in both launch
orders (run_last: the operator's launch runs after its output neighbours', so what it writes past its slice shows).  Bytes against the
oracle, exact; no concat_copy_i8 in the launch list proves that the slices were in effect."""
import functools

import numpy as np
import pytest

import test_gpu_gemm_family as fam
from oracle import oracle
from slice_helpers import GEMM_SHAPES, PGEMM_W_MEMBERS, gemm_case, gemm_eltwise_case
from tengine_amd import capi, tm2

pytestmark = pytest.mark.gpu

ORDERS = [True, False]
# conv_igemm.hip: conv_igemm_kernel_name, by tile configuration -- "igemm<k>" pins configuration k
IGEMM_NAMES = ["conv_igemm_i8<128x128x64>", "conv_igemm_i8<128x32x64>", "conv_igemm_i8<64x64x64>", "conv_igemm_i8<32x128x64>",
               "conv_igemm_i8<128x64x64>", "conv_igemm_i8<128x128x256>", "conv_igemm_i8<128x64x256>", "conv_igemm_i8<64x64x256>",
               "conv_igemm_i8<64x64x128>", "conv_igemm_i8<128x64x128>", "conv_igemm_i8<128x128x64,ring>", "conv_igemm_i8<128x64x64,ring>",
               "conv_igemm_i8<256x64x64,ring>", "conv_igemm_i8<64x128x64,ring>", "conv_igemm_i8<64x64x64,ring>", "conv_igemm_i8<256x128x64,ring>"]
ELT_MEMBERS = [m.args[1] for m in fam.test_fused_eltwise_tail_is_exact_in_every_member.pytestmark if m.args[0] == "member"][0]
# the issue's two shapes, and "big": conv_igemm2 wants 64 blocks of 128 pixels, which neither of the two has
ELT_SHAPES = ["pw_many", "k3", "big"]
USED = {}          # (member, run_last) -> the shapes on which the profile named the member


def is_member(member, kernel):
    if member.startswith("igemm"):
        return kernel.split("+")[0] == IGEMM_NAMES[int(member[5:])]
    return member in kernel


@functools.lru_cache(maxsize=None)
def case(shape, run_last):
    g, x = gemm_case(shape, run_last)
    want = oracle.run_graph(g, x)
    for w in want:
        w.setflags(write=False)
    return tm2.write_tm2(g), x, want


@functools.lru_cache(maxsize=None)
def eltwise_case(shape):
    g, x = gemm_eltwise_case(shape)
    want = oracle.run_graph(g, x)
    return tm2.write_tm2(g), x, want


def device(b, x, member, monkeypatch):
    monkeypatch.setenv("TAMD_FORCE_GEMM", member)
    gr = capi.Graph(b)
    gr.set_input(x)
    got = gr.run()
    prof = gr.profile(1)
    gr.close()
    return got, prof


def check(member, shape, run_last, monkeypatch):
    b, x, want = case(shape, run_last)
    got, prof = device(b, x, member, monkeypatch)
    names = [k["kernel"] for k in prof]
    kernel = [k["kernel"] for k in prof if k["node"] == "op"]
    assert names.count("concat_copy_i8") == 0 and len(kernel) == 1, prof
    for i, (o, w) in enumerate(zip(got, want)):
        bad = np.argwhere(o.reshape(w.shape) != w)
        assert len(bad) == 0, "%s (%s) on %s, run_last=%s: output %d, %d of %d bytes differ, first at (n, c, y, x) = %s" % (
            member, kernel[0], shape, run_last, i, len(bad), w.size, bad[0].tolist())
    if is_member(member, kernel[0]):
        USED.setdefault((member, run_last), set()).add(shape)
        return True
    return False


@pytest.mark.parametrize("run_last", ORDERS, ids=["op_last", "op_first"])
@pytest.mark.parametrize("shape", [s for s in GEMM_SHAPES if s != "k3_wide"])
@pytest.mark.parametrize("member", fam.MEMBERS)
def test_family_member_on_slices(member, shape, run_last, monkeypatch):
    """where the pinned member does not apply the planner falls back to the race: the bytes are compared all the same, the census
    below counts the case only when the profile names the member"""
    check(member, shape, run_last, monkeypatch)


@pytest.mark.parametrize("run_last", ORDERS, ids=["op_last", "op_first"])
@pytest.mark.parametrize("member", sorted(PGEMM_W_MEMBERS))
def test_dedicated_3x3_form_on_slices(member, run_last, monkeypatch):
    assert check(member, PGEMM_W_MEMBERS[member], run_last, monkeypatch), "%s did not run" % member


@pytest.mark.parametrize("shape", ELT_SHAPES)
@pytest.mark.parametrize("member", ELT_MEMBERS)
def test_fused_eltwise_tail_behind_a_sliced_input(member, shape, monkeypatch):
    b, x, want = eltwise_case(shape)
    got, prof = device(b, x, member, monkeypatch)
    names = [k["kernel"] for k in prof]
    kernel = [k["kernel"] for k in prof if k["node"] == "op"]
    assert names.count("concat_copy_i8") == 0 and len(kernel) == 1 and "+eltwise" in kernel[0], prof
    for o, w in zip(got, want):
        assert np.array_equal(o.reshape(w.shape), w), (member, kernel, np.count_nonzero(o.reshape(w.shape) != w))
    if is_member(member, kernel[0]):
        USED.setdefault((member, "eltwise"), set()).add(shape)


def test_census_every_member_ran_on_slices_in_both_orders(monkeypatch):
    """every name of the family list was the kernel of the sliced node on at least one shape, in both launch orders (cases that were
    deselected in this run are run here)"""
    missing = []
    for member in fam.MEMBERS:
        for run_last in ORDERS:
            for shape in GEMM_SHAPES:
                if USED.get((member, run_last)):
                    break
                check(member, shape, run_last, monkeypatch)
            if not USED.get((member, run_last)):
                missing.append((member, run_last))
    print("members by shape:", {m: sorted(s) for (m, r), s in sorted(USED.items(), key=str) if r is True})
    assert not missing, missing
    # the eltwise tail: every member the family's own tail test lists took it on a sliced input
    for member in ELT_MEMBERS:
        if not USED.get((member, "eltwise")):
            for shape in ELT_SHAPES:
                test_fused_eltwise_tail_behind_a_sliced_input(member, shape, monkeypatch)
        assert USED.get((member, "eltwise")), member
