// Two slots behind one handle: two passes in flight on two HSA queues (tamd_options.split_batch; graph_slots.h holds the arithmetic).
//
// Why: at batch 1 a pass is a chain of fourteen dependent packets, each a few hundred waves on 256 CUs -- the machine is idle, not
// full, and the chain itself has been worked over for seven rounds.  But the passes a caller queues one behind the
// other (bench.py's K steps, a server's images) are independent of each other: pass k + 1 reads nothing pass k writes, except that
// one launch list reuses one set of activation buffers.  Two graphs of the same model on two queues, launched alternately, run 27.7 us
// per pass against 49.2 for one (tools/exp/two_graphs_b1.py, profiles/two_slots_ab.txt) -- this file is that, behind ONE handle with
// ONE set of packed weights.
//
// How: slot 0 is the graph as it always was.  Slot 1 is a second DirectProgram of the same recorded launch list on a queue of its own,
// with everything a pass WRITES re-pointed at a private copy: every Step::wr range, every non-constant tensor's buffer, the outputs'
// staging buffers (which is also what the layout launches write).  The graph inputs' staging buffers are shared -- passes only read
// them, and everything that writes them drains both queues first -- as are weights, per-channel vectors and tables.  The launch
// records of slot 1 are copies of slot 0's in which every 8-byte argument word that points into a written span has moved by that
// span's distance (patch_pointer of graph_exec.hip is the precedent, and so is its rule: a patched program proves itself before use).
//
// What keeps results where they were: tamd_graph_launch alternates, direct_drain waits for both queues and hands the turn back to
// slot 0.  Every entry point that changes an input or reads a tensor drains first, so slot 0 runs first after every drain, every pass
// between two drains computes the same bytes, and slot 0's tensors and output buffers hold the current input's result whenever any
// pass has run: tamd_graph_output_device stays a persistent view, download / read_tensor / run / run_async never look at slot 1.
//
// It raises throughput (images/s).  It does not shorten a pass: tamd_graph_run, a lone launch + sync, tamd_graph_time_launches and
// tamd_graph_direct_timestamps (slot 0 alone) are what they were.
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace tamd {

namespace {

void say(const char* why)
{
    if (getenv("TAMD_DEBUG")) fprintf(stderr, "[tamd] slots: the graph stays one launch list: %s\n", why);
}

void add_access(std::vector<SlotRange>& r, const Access& a) { r.push_back(slot_range_of(a)); }

// The proof, in the scheme of direct_selfcheck.  (a) slot 1 ALONE reproduces the eager pass of input A byte for byte in its own output
// copies while slot 0's buffers hold input B's results -- a read pointer that was not moved shows as B's bytes, a write pointer that
// was not moved as A's bytes in slot 0.  (b) one burst of 8 alternating passes leaves A's results in both slots' outputs.
int slots_selfcheck(tamd_graph* g)
{
    OutputBytes want, other, got;
    if (selfcheck_fill_inputs(g, 0x51075A11u) || run_steps(g, g->stream)) return -1;
    HIPCHK(hipStreamSynchronize(g->stream));
    if (selfcheck_snapshot(g, &want)) return -1;
    if (selfcheck_fill_inputs(g, 0x0DDBA11Au) || run_steps(g, g->stream)) return -1;
    HIPCHK(hipStreamSynchronize(g->stream));
    if (selfcheck_snapshot(g, &other)) return -1;
    if (selfcheck_fill_inputs(g, 0x51075A11u)) return -1;
    HIPCHK(hipDeviceSynchronize());
    if (direct_submit(g->direct1) || direct_wait(g->direct1)) { set_error("the pass of slot 1 failed: %s", direct_last_error()); return -1; }
    if (selfcheck_snapshot(g, &got, -1, &g->slot_spans)) return -1;
    if (selfcheck_same(want, got, "slot 1 alone does not reproduce the eager pass (output %zu differs)")) return -1;
    if (selfcheck_snapshot(g, &got)) return -1;
    if (selfcheck_same(other, got, "the pass of slot 1 changed slot 0's output %zu")) return -1;
    for (int k = 0; k < 8; k++)
        if (direct_submit((k & 1) ? g->direct1 : g->direct)) { set_error("the alternating burst failed: %s", direct_last_error()); return -1; }
    if (direct_wait(g->direct) || direct_wait(g->direct1)) { set_error("the alternating burst failed: %s", direct_last_error()); return -1; }
    if (selfcheck_snapshot(g, &got)) return -1;
    if (selfcheck_same(want, got, "a burst of alternating passes leaves other bytes in slot 0 (output %zu differs)")) return -1;
    if (selfcheck_snapshot(g, &got, -1, &g->slot_spans)) return -1;
    if (selfcheck_same(want, got, "a burst of alternating passes leaves other bytes in slot 1 (output %zu differs)")) return -1;
    for (auto& io : g->inputs) HIPCHK(hipMemset(io.stage, 0, io.bytes));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

}  // namespace

// mode: tamd_options.split_batch after TAMD_SPLIT_BATCH -- 0 the default rule, 2 wherever a list qualifies (1 never reaches this).
// `recs`: the recorded launch list g->direct was built from.
void slots_try_build(tamd_graph* g, const std::vector<LaunchRec>& recs, int mode)
{
    if (!g->direct || g->is_half || g->inputs.empty() || g->outputs.empty()) { if (!g->direct) say("the list is not dispatched directly"); return; }
    // int8 graphs only: their launchers were audited -- none keeps a device workspace or a counter of its own, everything a launch
    // writes is a tensor or stands in its wr (the uint8 / fp32 planners' fp32 copies and Winograd workspaces were not looked at for this)
    for (auto& t : g->tensors)
        if (t.ttype != TAMD_TT_CONST && t.dtype != TAMD_DT_INT8) { say("not an int8 graph"); return; }
    if (mode != 2) {       // the default rule: where it was measured to pay -- batch 1 (profiles/two_slots_ab.txt)
        const HTensor& in0 = g->tensors[g->inputs[0].tensor];
        if (in0.dims.empty() || in0.dims[0] != 1) return;
    }
    if (g->had_once) { say("a launch of the plan ran once at prerun (its results exist in one copy)"); return; }
    for (auto& st : g->steps)
        if (step_states_nothing(st)) { say("a launch states nothing of what it reads and writes"); return; }
    // what a pass writes
    std::vector<SlotRange> ranges;
    for (auto* v : {&g->in_steps, &g->steps, &g->out_steps})
        for (auto& st : *v)
            for (auto& w : st.wr) add_access(ranges, w);
    auto is_input_stage = [&](const void* p) {
        for (auto& io : g->inputs)
            if ((const char*)p >= (const char*)io.stage && (const char*)p < (const char*)io.stage + io.bytes) return true;
        return false;
    };
    for (auto& t : g->tensors)
        if (t.ttype != TAMD_TT_CONST && t.dptr && !t.prerun_const && !is_input_stage(t.dptr)) add_access(ranges, access_of(t));
    for (auto& io : g->outputs) {
        SlotRange x;
        x.lo = (uintptr_t)io.stage; x.bytes = io.bytes;
        ranges.push_back(x);
    }
    // a range never leaves the allocation it begins in (a reshaped alias describes its owner's bytes with its own geometry)
    for (auto& x : ranges)
        for (auto& a : g->arenas)
            if (x.lo >= (uintptr_t)a.base && x.lo < (uintptr_t)a.base + a.used) x.bytes = std::min<size_t>(x.bytes, (uintptr_t)a.base + a.used - x.lo);
    size_t total = 0;
    std::vector<SlotSpan> spans = slot_merge(ranges, &total);
    if (spans.empty()) { say("nothing to re-point"); return; }
    for (auto& io : g->inputs)
        if (slot_touches(spans, (uintptr_t)io.stage, io.bytes)) { say("a launch writes a graph input's staging buffer"); return; }
    for (auto& t : g->tensors)
        if (t.prerun_const && t.dptr && slot_touches(spans, (uintptr_t)t.dptr, 1)) { say("a prerun constant lives in a written buffer"); return; }
    if (hipMalloc(&g->slot_block, total) != hipSuccess) { (void)hipGetLastError(); g->slot_block = nullptr; say("no device memory for the second slot"); return; }
    slot_place(spans, (uintptr_t)g->slot_block);
    // the copy starts as slot 0 is: padding channels (zero from the allocation on) and anything else prerun left in those bytes
    bool ok = hipMemset(g->slot_block, 0, total) == hipSuccess;
    for (size_t i = 0; i < spans.size() && ok; i++)
        ok = hipMemcpy((char*)g->slot_block + spans[i].off, (const void*)spans[i].lo, spans[i].hi - spans[i].lo, hipMemcpyDeviceToDevice) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { (void)hipGetLastError(); say("the copy of the written spans failed"); slots_destroy(g); return; }
    std::vector<LaunchRec> recs1 = recs;
    int moved = 0;
    for (auto& r : recs1) moved += slot_rebase(r.args.data(), r.args.size(), spans);
    if (!moved) { say("no argument points into a written span"); slots_destroy(g); return; }
    const char* why = "";
    g->direct1 = direct_build(g->gpu, g->stream, recs1, &why);          // no `share`: a queue of its own
    if (!g->direct1) { say(why); slots_destroy(g); return; }
    g->slot_spans = spans;
    if (slots_selfcheck(g)) {
        fprintf(stderr, "tengine_amd: the second slot is NOT used for this graph: %s (one launch list, as before)\n", last_error());
        slots_destroy(g);
        return;
    }
    if (getenv("TAMD_DEBUG"))
        fprintf(stderr, "[tamd] slots: two passes in flight on two HSA queues; slot 1 owns %zu span(s), %.2f MB, %d argument words re-pointed in %zu launches\n",
                spans.size(), total / 1048576.0, moved, recs1.size());
}

void slots_destroy(tamd_graph* g)
{
    if (g->direct1) { direct_destroy(g->direct1); g->direct1 = nullptr; }       // (waits for what still runs, bounded: direct.cc)
    if (g->slot_block) { (void)hipFree(g->slot_block); g->slot_block = nullptr; }
    g->slot_spans.clear();
    g->slot_turn = 0;
}

// raw stamps of one burst of alternating passes on both queues (direct.cc direct_timestamps_two)
int slots_timestamps(tamd_graph* g, int passes, double* start_us, double* end_us, int max_stamps)
{
    if (!g->direct || !g->direct1) { set_error("tamd_graph_slot_timestamps: the graph has one launch list (tamd_graph_slots() == 0)"); return -1; }
    const int n = direct_packets(g->direct);
    if (passes < 1 || (long long)passes * 2 * n > (long long)max_stamps) { set_error("tamd_graph_slot_timestamps: %d rounds of 2 x %d packets, room for %d stamps", passes, n, max_stamps); return -1; }
    const int rc = direct_timestamps_two(g->direct, g->direct1, passes, start_us, end_us);
    if (rc < 0) { set_error("direct dispatch: %s", direct_last_error()); return -1; }
    return rc;
}

}  // namespace tamd
