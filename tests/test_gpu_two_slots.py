"""Two slots behind one handle (tamd_options.split_batch, csrc/graph_slots.hip): an int8 graph dispatched directly at batch 1 keeps two
passes of its one launch list in flight on two HSA queues.  Which graphs take the form, and that nothing a caller can see changes: the
bytes of every run path against the one-list form and the oracle, the persistent view of the outputs, intermediate tensors, a close
right behind a burst."""
import numpy as np
import pytest

from helpers import _scales, u8_conv_graph
from oracle import oracle
from tengine_amd import capi, models, plans, tm2
from tengine_amd.tm2 import DT_INT8, DT_INT32
from test_gpu_direct import hip_runtime_of_the_library

pytestmark = pytest.mark.gpu


def small_graph(batch=1, seed=11):
    """3x3 stride-2 conv on 3x16x16 -> dw 3x3 + pw (8 -> 16) -> dw 3x3 stride 2 + pw (16 -> 16) -> global average pool -> FC to 10"""
    rng = np.random.default_rng(seed)
    g = tm2.Graph(name="two_slots_case")
    xs = float(np.float32(rng.uniform(0.01, 0.05)))
    cur = g.add_input("data", [batch, 3, 16, 16], DT_INT8, [xs], [0])
    cs, ch, hw = xs, 3, 16

    def conv(name, x, cout, k, s, p, group, in_scale, cin, size):
        wq = rng.integers(-127, 128, size=(cout, cin // group, k, k)).astype(np.int8)
        ws = _scales(rng, cout)
        ins = [x, g.add_const(name + "/w", wq, DT_INT8, ws, [0] * cout),
               g.add_const(name + "/b", rng.integers(-2000, 2000, size=(cout,)).astype(np.int32), DT_INT32, [1.0], [0])]
        out = (size + 2 * p - k) // s + 1
        os_ = float(np.float32(in_scale * np.mean(ws) * 73.0 * np.sqrt((cin // group) * k * k) * 73.0 / 60.0))
        y = g.add_tensor(name + "/0", [batch, cout, out, out], DT_INT8, tm2.TT_VAR, None, [os_], [0])
        g.add_node(name, "Convolution", ins, [y], input_channel=cin, output_channel=cout, group=group, activation=0, kernel_h=k, kernel_w=k,
                   stride_h=s, stride_w=s, dilation_h=1, dilation_w=1, pad_h0=p, pad_w0=p, pad_h1=p, pad_w1=p)
        return y, os_, out

    cur, cs, hw = conv("conv1", cur, 8, 3, 2, 1, 1, cs, ch, hw)
    ch = 8
    for tag, cout, s in (("2", 16, 1), ("3", 16, 2)):
        cur, cs, hw = conv("conv%s/dw" % tag, cur, ch, 3, s, 1, ch, cs, ch, hw)
        cur, cs, hw = conv("conv%s/sep" % tag, cur, cout, 1, 1, 0, 1, cs, ch, hw)
        ch = cout
    ps = float(np.float32(cs * 0.6))
    pooled = g.add_tensor("pool/0", [batch, ch, 1, 1], DT_INT8, tm2.TT_VAR, None, [ps], [0])
    g.add_node("pool", "Pooling", [cur], [pooled], alg=tm2.POOL_AVG, kernel_h=hw, kernel_w=hw, stride_h=1, stride_w=1, **{"global": 1}, caffe_flavor=0,
               pad_h0=0, pad_w0=0, pad_h1=0, pad_w1=0)
    wq = rng.integers(-127, 128, size=(10, ch)).astype(np.int8)
    ws = _scales(rng, 10)
    ins = [pooled, g.add_const("fc/w", wq, DT_INT8, ws, [0] * 10), g.add_const("fc/b", rng.integers(-2000, 2000, size=(10,)).astype(np.int32), DT_INT32, [1.0], [0])]
    y = g.add_tensor("fc/0", [batch, 10], DT_INT8, tm2.TT_VAR, None, [float(np.float32(ps * np.mean(ws) * 73.0 * np.sqrt(ch) * 73.0 / 60.0))], [0])
    g.output_nodes = [g.add_node("fc", "FullyConnected", ins, [y], num_output=10)]
    return g


def inputs_of(g, seeds=(5, 6, 7)):
    dims = g.tensors[g.nodes[g.input_nodes[0]].outputs[0]].dims
    return [np.random.default_rng(s).integers(-127, 128, size=dims).astype(np.int8) for s in seeds]


@pytest.fixture(scope="module")
def small():
    """the small graph, three inputs and the oracle's output for each -- computed once, shared, never changed"""
    g = small_graph(1)
    xs = inputs_of(g)
    want = [oracle.run_graph(g, x)[0] for x in xs]
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])      # a stale slot would show
    return g, tm2.write_tm2(g), xs, want


def device_bytes(ptr, nbytes):
    back = np.zeros(nbytes, np.uint8)
    assert hip_runtime_of_the_library().hipMemcpy(back.ctypes.data, ptr, nbytes, 2) == 0
    return back


def test_which_graphs_take_two_slots(small, monkeypatch):
    g, b, xs, want = small
    two = capi.Graph(b, direct_dispatch=True)
    one = capi.Graph(b, direct_dispatch=True, split_batch=1)
    assert two.slots() == 2 and one.slots() == 0
    assert two.halves() == 0 and one.halves() == 0
    assert two.direct_packets() == one.direct_packets() > 0          # the per-pass count, in both forms
    assert two.kernel_num() == one.kernel_num()
    two.close(); one.close()
    off = capi.Graph(b, direct_dispatch=False)
    assert off.slots() == 0 and off.direct_packets() == 0
    off.close()
    wherever = capi.Graph(b, direct_dispatch=True, split_batch=2)
    assert wherever.slots() == 2 and wherever.halves() == 0
    wherever.close()
    b2 = tm2.write_tm2(small_graph(2))
    at2 = capi.Graph(b2, direct_dispatch=True)
    assert at2.slots() == 0 and at2.halves() == 0                    # the default rule: batch 1 only
    at2.close()
    gu, _ = u8_conv_graph(5, 1, 16, 9, 9, 24, 3, 1, 1)
    u8 = capi.Graph(tm2.write_tm2(gu), direct_dispatch=True)
    assert u8.slots() == 0
    u8.close()
    monkeypatch.setenv("TAMD_SPLIT_BATCH", "0")
    never = capi.Graph(b, direct_dispatch=True)
    assert never.slots() == 0
    never.close()


def test_bursts_give_the_one_list_forms_bytes_and_the_view_stays(small):
    g, b, xs, want = small
    two = capi.Graph(b, direct_dispatch=True)
    one = capi.Graph(b, direct_dispatch=True, split_batch=1)
    assert two.slots() == 2 and one.slots() == 0
    ptr, nbytes = two.output_device(0)                  # taken ONCE, before any pass
    k = 0
    for burst in (1, 2, 3, 4, 5, 2, 1):
        x, w = xs[k % 3], want[k % 3]
        k += 1
        for gr in (two, one):
            gr.set_input(x); gr.upload()
            for _ in range(burst):
                gr.launch()
            gr.sync()
        got, ref = two.download()[0], one.download()[0]
        assert np.array_equal(got, ref), "burst of %d" % burst
        assert np.array_equal(got.reshape(w.shape), w), "burst of %d against the oracle" % burst
        assert np.array_equal(device_bytes(ptr, nbytes), got.view(np.uint8).reshape(-1)), "the persistent view after a burst of %d" % burst
        assert two.output_device(0) == (ptr, nbytes)
    # a second burst on the SAME input without an upload in between (the turn went back to slot 0 at the sync)
    two.launch(); two.launch(); two.launch(); two.sync()
    assert np.array_equal(device_bytes(ptr, nbytes), one.download()[0].view(np.uint8).reshape(-1))
    two.close(); one.close()


def test_intermediate_tensors_after_odd_and_even_bursts(small):
    g, b, xs, want = small
    two = capi.Graph(b, direct_dispatch=True, keep_tensors=True)
    one = capi.Graph(b, direct_dispatch=True, keep_tensors=True, split_batch=1)
    assert two.slots() == 2 and one.slots() == 0
    one.set_input(xs[0]); one.upload(); one.launch(); one.sync()
    readable = []
    for ti, t in enumerate(g.tensors):
        if t.ttype != tm2.TT_VAR or t.name == "fc/0":
            continue
        try:
            one.read_tensor(ti)
            readable.append(ti)
        except capi.TamdError:
            pass                                        # fused into its consumer's launch: never reaches memory in either form
    assert readable, "no intermediate tensor of the small graph reaches memory"
    for k, burst in enumerate((3, 2, 1, 4)):
        x = xs[(k + 1) % 3]
        for gr in (two, one):
            gr.set_input(x); gr.upload()
            for _ in range(burst):
                gr.launch()
        for ti in readable:                             # (read_tensor waits for the passes itself)
            assert np.array_equal(two.read_tensor(ti), one.read_tensor(ti)), "%s after a burst of %d" % (g.tensors[ti].name, burst)
    two.close(); one.close()


def test_mixed_paths_and_a_close_behind_a_burst(small):
    g, b, xs, want = small
    two = capi.Graph(b, direct_dispatch=True)
    assert two.slots() == 2
    shape = want[0].shape
    two.set_input(xs[0]); two.upload()
    for _ in range(3):
        two.launch()
    two.set_input(xs[1])
    assert np.array_equal(two.run()[0].reshape(shape), want[1])                      # launches, then run() ...
    two.set_input(xs[2]); two.upload()
    for _ in range(2):
        two.launch()
    two.sync()
    assert np.array_equal(two.download()[0].reshape(shape), want[2])                 # ... then launches
    outs = [two.output_like(), two.output_like()]
    two.set_input(xs[0]); two.run_async(outs[0])
    two.set_input(xs[1]); two.run_async(outs[1])
    two.wait(); two.wait()
    two.bind_default_outputs()
    assert np.array_equal(outs[0][0].reshape(shape), want[0]) and np.array_equal(outs[1][0].reshape(shape), want[1])
    two.set_input(xs[2]); two.upload()
    for _ in range(5):
        two.launch()
    two.sync()
    assert np.array_equal(two.download()[0].reshape(shape), want[2])
    # the chain's own figure runs slot 0 alone and leaves the form as it was
    assert two.time_launches(4) > 0
    assert np.array_equal(two.download()[0].reshape(shape), want[2]) and two.slots() == 2
    two.set_input(xs[0]); two.upload()
    for _ in range(7):
        two.launch()
    two.close()                                          # right behind a burst, no sync: both queues are drained by the close


def test_mobilenet_v1_batch_1(tmp_path, monkeypatch):
    plan = str(tmp_path / "plan.txt")
    plans.seed(plan, "mobilenet_v1", "int8", 1)         # the shipped plan: no plan-time races in a test
    monkeypatch.setenv("TAMD_PLAN_CACHE", plan)
    g = models.build("mobilenet_v1", "int8", 1)
    b = tm2.write_tm2(g)
    xs = [models.synth_input(g, s) for s in (7, 8)]
    want = oracle.run_graph(g, xs[0])[0]
    two = capi.Graph(b, direct_dispatch=True)
    one = capi.Graph(b, direct_dispatch=True, split_batch=1)
    assert two.slots() == 2 and one.slots() == 0 and two.direct_packets() == one.direct_packets()
    ptr, nbytes = two.output_device(0)
    for x, burst in ((xs[1], 4), (xs[0], 5)):
        for gr in (two, one):
            gr.set_input(x); gr.upload()
            for _ in range(burst):
                gr.launch()
            gr.sync()
        got = two.download()[0]
        assert np.array_equal(got, one.download()[0])
        assert np.array_equal(device_bytes(ptr, nbytes), got.view(np.uint8).reshape(-1))
    assert np.array_equal(got.reshape(want.shape), want)
    two.close(); one.close()


_STAMPS = r"""
import os, sys
sys.path.insert(0, %r)
import numpy as np
from tengine_amd import capi, models, plans, tm2
plans.seed(os.environ["TAMD_PLAN_CACHE"], "mobilenet_v1", "int8", 1)
g = models.build("mobilenet_v1", "int8", 1)
gr = capi.Graph(tm2.write_tm2(g), direct_dispatch=True)
assert gr.slots() == 2
gr.set_input(models.synth_input(g, 1, tm2.DT_INT8))
gr.upload(); gr.launch(); gr.sync()
before = gr.download()[0]
n = gr.direct_packets()
rows = gr.direct_timestamps(30)                          # slot 0 alone: the chain as it is
assert len(rows) == n and all(d > 0.2 for _, d, _ in rows), rows
assert all(gp > -0.05 for _, _, gp in rows), rows       # one in-order queue: no packet starts before its predecessor ends
t0, t1 = gr.slot_timestamps(30)                          # one burst of alternating passes, both queues stamped
assert 1 <= t0.shape[0] <= 30 and t0.shape[1:] == (2, n) and (t1 > t0).all() and t0.min() == 0.0
for slot in (0, 1):                                      # each queue is an in-order chain of its own ...
    s0, s1 = t0[:, slot, :].reshape(-1), t1[:, slot, :].reshape(-1)
    assert (s0[1:] > s1[:-1] - 0.05).all()
both = sum(min(b, d) - max(a, c) > 0 for a, b in zip(t0[:, 0, :].reshape(-1), t1[:, 0, :].reshape(-1))
           for c, d in zip(t0[:, 1, :].reshape(-1), t1[:, 1, :].reshape(-1)))
assert both > 0                                          # ... and packets of the two queues do run at the same time
assert np.array_equal(gr.download()[0], before) and gr.slots() == 2
print("STAMPS %%d packets per pass, %%d rounds stamped on both queues, %%d overlapping packet pairs" %% (n, t0.shape[0], both))
gr.close()
"""


def test_stamps_of_the_chain_and_of_a_burst_on_both_queues(tmp_path):
    """tamd_graph_direct_timestamps keeps stamping slot 0 alone; tamd_graph_slot_timestamps stamps one burst of alternating passes on both
    queues, raw, on the common clock.  In a process of its own, as tools/direct_timestamps.py uses them (in a process that has created and
    destroyed hundreds of HSA queues stamped passes have come back without stamps: tests/test_gpu_split_batch.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, TAMD_PLAN_CACHE=str(tmp_path / "plan.txt"))
    e.pop("TAMD_SPLIT_BATCH", None)
    e.pop("TAMD_DIRECT_DISPATCH", None)
    r = subprocess.run([sys.executable, "-c", _STAMPS % root], capture_output=True, text=True, env=e, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STAMPS")]
    assert r.returncode == 0 and line, (r.stdout[-800:], r.stderr[-2000:])
    print(line[0])
