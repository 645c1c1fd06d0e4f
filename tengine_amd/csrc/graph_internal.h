// What the translation units of the graph layer share (private).  The layer is eleven units:
//   graph.hip             the C ABI that builds, describes, pre-runs, profiles, reads and destroys a graph
//   graph_infer.hip       shape inference, validation, the PriorBox evaluator, the error string
//   graph_plan_common.hip what every planner shares: dev_alloc (arena), tensor geometry, the NCHW planners' buffer front and output
//                         tail, axis_split, conv_tap_table, and append_steps: the one place that appends a launch and checks what it
//                         says it reads and writes
//   graph_plan.hip        the int8 planner (layout passes, one function per node kind, plan_i8)
//   graph_plan_conv.hip   .. its convolution / FC / pooling launches (requantisation folds, packers, one function per conv form)
//   graph_plan_pairs.hip  .. its fusions (pwdw, chain4, dwpw, the bottleneck block)
//   graph_plan_maps.hip   the byte-map node planners (tables, PReLU, nearest Interp, Split / ShuffleChannel), int8 and uint8 forms;
//                         graph_plan.h is what the int8 units share
//   plan_cache.hip        TAMD_PLAN_CACHE
//   graph_pair.hip        a batched graph as two half-batch graphs side by side behind one handle (tamd_options.split_batch)
//   graph_slots.hip       one launch list as two slots on two HSA queues: two passes in flight (graph_slots.h: the host-only arithmetic)
//   graph_exec.hip        run_steps, the direct path's self-checks, zero-copy lists, the run-side entry points
//   graph_u8.hip, graph_f32.hip   the uint8 / fp32 planners (plan_u8, plan_f32): dense NCHW tensors
// node_rules.h (through graph.h) states once the node-local rules that the support query, validate_graph and the planners share.
#pragma once
#include <mutex>

#include "graph.h"
#include "launch_rec.h"

namespace tamd {

// prerun (plan + hipGraph capture) and the device-synchronous frees are serialised process-wide (graph_infer.hip)
extern std::mutex g_capture_mutex;
const char* last_error();                    // the calling thread's error string (set_error)

static inline int esize(int dt) { return (dt == TAMD_DT_FP32 || dt == TAMD_DT_INT32) ? 4 : (dt == TAMD_DT_FP16 ? 2 : 1); }
static inline int cdiv_c(int a, int b) { return a / b; }  // C semantics (truncation), as the reference

int infer_shapes(tamd_graph* g);             // graph_infer.hip
int validate_graph(tamd_graph* g);
int plan_i8(tamd_graph* g);                  // graph_plan.hip: every activation tensor is int8
void plan_cache_flush();                     // plan_cache.hip

// graph_exec.hip
int run_steps(tamd_graph* g, hipStream_t s, int io_slot = -1);
// one eager pass of run_steps for I/O slot `io_slot` (-1: the launch list alone) with the launch recorder on (launch_rec.h), into *recs
int record_pass(tamd_graph* g, int io_slot, std::vector<LaunchRec>* recs);
int direct_selfcheck(tamd_graph* g);
// what the self-checks share (direct_selfcheck, direct_io_selfcheck; slots_selfcheck of graph_slots.hip).  Seeded pseudo-random bytes
// (finite floats) into every graph input: its device staging buffer, or with io_slot >= 0 that I/O slot's pinned buffer
int selfcheck_fill_inputs(tamd_graph* g, unsigned seed, int io_slot = -1);
// a copy of every graph output: from its staging buffer, from where the pass-slot span map `spans` moved that buffer, or with
// io_slot >= 0 from that I/O slot's pinned buffer
typedef std::vector<std::vector<unsigned char>> OutputBytes;
int selfcheck_snapshot(const tamd_graph* g, OutputBytes* dst, int io_slot = -1, const std::vector<SlotSpan>* spans = nullptr);
// -1 and the error `fmt` (which takes the output's index as its one %zu) at the first output whose bytes differ
int selfcheck_same(const OutputBytes& want, const OutputBytes& got, const char* fmt);
// g->io[io_slot].direct / .zero_copy: the host-to-host list of that I/O slot as a program on g->direct's queue, outputs stored straight
// into the pinned buffers where the list allows it and the program proves itself.  -1: a HIP error; no program is no error
int build_io_program(tamd_graph* g, int io_slot);
int bind_device(tamd_graph* g);
int direct_drain(tamd_graph* g);
void direct_teardown(tamd_graph* g);         // the I/O slots' programs, the second pass slot, g->direct: waits for what still runs (direct.cc)
int stage_from_pinned(tamd_graph* g);

// graph_slots.hip: two passes in flight on two HSA queues behind one handle (tamd_options.split_batch)
void slots_try_build(tamd_graph* g, const std::vector<LaunchRec>& recs, int mode);   // never an error: the graph stays one list when anything is in the way
void slots_destroy(tamd_graph* g);           // waits for slot 1's passes, then releases its program, queue and memory
int slots_timestamps(tamd_graph* g, int passes, double* start_us, double* end_us, int max_stamps);

// graph_pair.hip: a batched graph as two half-batch device graphs behind one tamd_graph (tamd_options.split_batch); every entry point
// of the C ABI forwards to these when g->half[0] is set
int pair_try_prerun(tamd_graph* g, const tamd_options* opt);     // 0: stays one launch list; 1: a pair now, prepared; < 0: error
int pair_set_input(tamd_graph* g, int idx, const void* host, size_t bytes);
int pair_set_output(tamd_graph* g, int idx, void* host, size_t bytes);
int pair_both(tamd_graph* g, int (*fn)(tamd_graph*));
int pair_run(tamd_graph* g);
int pair_run_async(tamd_graph* g);
int pair_wait(tamd_graph* g);
int pair_direct_packets(const tamd_graph* g, bool meta);
const char* pair_direct_packet_name(const tamd_graph* g, int i);
int pair_direct_timestamps(tamd_graph* g, int passes, double* dur_us, double* gap_us, int max_packets);
int pair_output_device(tamd_graph* g, int idx, void** dptr, size_t* bytes);
int pair_time_launches(tamd_graph* g, int iters, float* total_ms);
int pair_kernel_num(const tamd_graph* g);
int pair_profile(tamd_graph* g, int iters, tamd_kernel_info* out, int max_out);
int pair_read_tensor(tamd_graph* g, int idx, void* host, size_t bytes);
void pair_destroy(tamd_graph* g);

// One graph = one thread at a time: every entry point that changes the graph or touches its buffers holds the graph for the
// duration of the call (nested entry points of the SAME thread pass).  Calls from different threads one after the other are fine --
// Tengine's scheduler does that -- two at once are a caller's bug that used to show up as corrupted launch lists; now the second
// call fails with an error.
struct OneThread {
    tamd_graph* g;
    bool ok = true, outer = false;
    explicit OneThread(tamd_graph* g_) : g(g_)
    {
        static thread_local char marker;
        const unsigned long me = (unsigned long)(uintptr_t)&marker;
        if (!g) return;
        unsigned long none = 0;
        if (g->owner.compare_exchange_strong(none, me)) outer = true;
        else if (none != me) ok = false;
    }
    ~OneThread() { if (g && outer) g->owner.store(0); }
};

}  // namespace tamd

#define TAMD_ONE_THREAD(g_)                                                                                                          \
    tamd::OneThread one_thread_(g_);                                                                                                 \
    if (!one_thread_.ok) { tamd::set_error("this tamd_graph is inside a call on another thread: one graph = one thread at a time (include/tengine_amd.h)"); return -1; }
