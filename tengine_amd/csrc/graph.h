// Host-side graph IR, planner and executor of the backend (private).
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <atomic>
#include <map>
#include <string>
#include <vector>

#include "../../include/tengine_amd.h"
#include "graph_slots.h"
#include "kernels.h"
#include "node_rules.h"

namespace tamd {

void set_error(const char* fmt, ...);
static inline int rup(int v, int m) { return (v + m - 1) / m * m; }

struct HTensor {               // host IR tensor == the parts of struct tensor the backend reads
    int dtype = 0, ttype = TAMD_TT_VAR;
    std::vector<int> dims;     // NCHW etc.
    std::vector<uint8_t> data; // const payload (copied)
    std::vector<float> scales;
    std::vector<int> zps;
    std::string name;
    // device view (valid after prerun for var/input tensors)
    void* dptr = nullptr;      // base of the NHWC buffer this tensor lives in
    int n = 0, h = 0, w = 0, c = 0;
    int cs = 0;                // channel stride of the *buffer* (bytes per pixel for int8)
    int c_off = 0;             // channel offset inside the buffer pixel (concat-by-offset views)
    bool is_view = false;      // aliases another tensor's buffer
    bool nchw_raw = false;     // graph input kept in NCHW for a direct first conv
    bool prerun_const = false; // written once at prerun (PriorBox and what only depends on it), never by a run
    size_t elems() const { size_t e = 1; for (int d : dims) e *= (size_t)d; return e; }
};

union NodeParam {
    tamd_conv_param conv;
    tamd_fc_param fc;
    tamd_pool_param pool;
    tamd_relu_param relu;
    tamd_eltwise_param elt;
    tamd_concat_param concat;
    tamd_upsample_param ups;
    tamd_permute_param perm;
    tamd_softmax_param softmax;
    tamd_reshape_param reshape;
    tamd_priorbox_param priorbox;
    tamd_clip_param clip;
    tamd_hardswish_param hardswish;
    tamd_interp_param interp;
    tamd_split_param split;
    tamd_shufflechannel_param shuffle;
    tamd_slice_param slice;
    tamd_transpose_param transpose;
    tamd_crop_param crop;
    tamd_depthtospace_param d2s;
    tamd_resize_param resize;
    tamd_batchnorm_param bn;
    tamd_instancenorm_param inorm;
};

struct HNode {
    int op = 0;
    std::vector<int> in, out;
    NodeParam p{};
    std::string name;
};

// what a step touches, for the dependency-aware barrier bits of the direct path: bytes [base, base + size) and, when period > 0,
// only the slice [off, off + len) of every `period` bytes (a concat input's slot, a channel range of an NCHW concat buffer)
struct Access {
    const char* base = nullptr;
    size_t size = 0, off = 0, len = 0, period = 0;
};
inline bool access_overlap(const Access& a, const Access& b)
{
    if (a.base + a.size <= b.base || b.base + b.size <= a.base) return false;
    if (a.base == b.base && a.size == b.size && a.period > 0 && a.period == b.period) return !(a.off + a.len <= b.off || b.off + b.len <= a.off);
    return true;
}

struct Step {                  // one device launch of the compiled plan
    std::string node, kernel;
    double macs = 0, bytes = 0;
    std::function<hipError_t(hipStream_t)> fn;
    bool once = false;         // every input is a prerun constant (PriorBox outputs): launched once at the end of prerun
    // rd / wr list EVERYTHING the step's launch reads / writes in device memory that another step may write (constants left
    // out) -- only then is deps set, and only a step with deps may run beside its predecessors (graph_exec.hip run_steps).  Every
    // compute step of every graph lists them, most without deps (they stay ordered): append_steps refuses a step that states
    // nothing and one whose wr overlaps its rd (graph_plan_common.hip)
    bool deps = false;
    std::vector<Access> rd, wr;
};
inline bool step_conflict(const Step& a, const Step& b)          // RAW, WAR or WAW between two steps that both carry deps
{
    for (auto& w : a.wr) { for (auto& x : b.wr) if (access_overlap(w, x)) return true; for (auto& x : b.rd) if (access_overlap(w, x)) return true; }
    for (auto& r : a.rd) for (auto& x : b.wr) if (access_overlap(r, x)) return true;
    return false;
}
inline bool step_states_nothing(const Step& s) { return s.rd.empty() || s.wr.empty(); }
inline bool step_writes_what_it_reads(const Step& s)             // any write against any read of the SAME launch
{
    for (auto& w : s.wr)
        for (auto& r : s.rd)
            if (access_overlap(w, r)) return true;
    return false;
}
// The one way to make a step: what the profile shows of it (node, kernel, macs, bytes), the launch, and what that launch reads and
// writes (rd / wr, see Step).  deps: the lists are complete AND the step may run beside its predecessors.  Without deps the lists change
// nothing at run time -- run_steps reads them only behind deps, the step stays ordered -- they are what append_steps' check reads.
// No defaults: only the layout launches (in_steps / out_steps) state nothing, and they say so with explicit empty lists
inline Step make_step(const std::string& node, const std::string& kernel, double macs, double bytes, std::function<hipError_t(hipStream_t)> fn,
                      std::vector<Access> rd, std::vector<Access> wr, bool deps)
{
    Step st;
    st.node = node; st.kernel = kernel; st.macs = macs; st.bytes = bytes; st.fn = std::move(fn);
    st.rd = std::move(rd); st.wr = std::move(wr); st.deps = deps;
    return st;
}
inline Access access_of(const HTensor& t)                         // dense tensor, or the channel slice of the concat buffer it lives in
{
    Access a;
    a.base = (const char*)t.dptr;
    const size_t esz = t.dtype == TAMD_DT_FP32 ? 4 : 1;
    if (t.nchw_raw || t.cs <= 0) {                                // NCHW bytes (uint8 / fp32 graphs, raw graph inputs)
        if (t.is_view && t.cs > 0) {
            a.period = (size_t)t.cs * t.h * t.w * esz; a.off = (size_t)t.c_off * t.h * t.w * esz; a.len = (size_t)t.c * t.h * t.w * esz;
            a.size = a.period * (size_t)t.n;
        } else {
            a.size = t.elems() * esz; a.len = a.size;
        }
    } else {                                                      // NHWC int8 buffer, cs bytes per pixel; a view owns channels [c_off, c_off + c)
        a.size = (size_t)t.n * t.h * t.w * t.cs;
        if (t.is_view) { a.period = (size_t)t.cs; a.off = (size_t)t.c_off; a.len = (size_t)t.c; }
        else a.len = a.size;
    }
    return a;
}
// raw bytes [p, p + bytes): a buffer that is no tensor (the fp32 copy of a uint8 tensor, the Winograd workspaces)
inline Access access_of_bytes(const void* p, size_t bytes)
{
    Access a;
    a.base = (const char*)p; a.size = bytes; a.len = bytes;
    return a;
}

// channels [first, first + count) of every pixel of the NHWC int8 buffer that `t` lives in, counted from t's own first channel: what
// access_of cannot say of a tensor that is no view (a concat input's slot of the concat's buffer)
inline Access access_of_channels(const HTensor& t, int first, int count)
{
    Access a;
    a.base = (const char*)t.dptr;
    a.size = (size_t)t.n * t.h * t.w * t.cs;
    a.period = (size_t)t.cs; a.off = (size_t)(t.c_off + first); a.len = (size_t)count;
    return a;
}
// elements [off, off + len) of every `period` elements of the dense tensor `y`, `esz` bytes per element: a concat input's slot of the
// NCHW planners' concat output (any axis: period = the output's elements per index in front of the axis)
inline Access access_of_slot(const HTensor& y, size_t period, size_t off, size_t len, size_t esz)
{
    Access a;
    a.base = (const char*)y.dptr;
    a.size = y.elems() * esz; a.period = period * esz; a.off = off * esz; a.len = len * esz;
    return a;
}

struct IOBind {
    int tensor = -1;
    const void* host_in = nullptr;   // re-read at every run
    void* host_out = nullptr;
    size_t bytes = 0;
    void* stage = nullptr;           // device buffer in the reference's NCHW order
    void* pinned[2] = {nullptr, nullptr};   // pinned host bounce buffers, one per I/O slot (IoSlot); allocated in tamd_graph_prerun
};

// One I/O slot of the host-to-host runs (tamd_graph_run: I/O slot 0; tamd_graph_run_async keeps two runs in flight, one per I/O slot):
// the launch list with the input upload in front and the output download behind it as copy KERNELS on the device-mapped pinned
// buffers IOBind::pinned[this slot].  Not the pass slots of graph_slots.hip, which is what "slot" alone means in this layer
struct IoSlot {
    DirectProgram* direct = nullptr; // that list as AQL packets on the HSA queue of tamd_graph::direct; nullptr: the hipGraph below
    bool zero_copy = false;          // .. and it stores the graph outputs straight into the pinned host buffers (no download launch)
    hipGraph_t hgraph = nullptr;     // the list as a captured graph, two instances launched round-robin (tamd_graph::hexecs says why)
    hipGraphExec_t hexec[2] = {nullptr, nullptr};
    int next_exec = 0;
    hipEvent_t done = nullptr;       // completion of an asynchronous run on the hipGraph path
};

struct Inflight {                    // one tamd_graph_run_async() that tamd_graph_wait() has not collected yet
    int io_slot = 0;
    std::vector<void*> host_out;     // where the caller wants this run's outputs (set_output at submit time)
    hipEvent_t done = nullptr;       // hipGraph path
    bool direct = false;             // direct path: the run is burst `burst` of the graph's HSA queue (direct.cc)
    unsigned long long burst = 0;
};

struct PoolGeom { int oh, ow, kh, kw, sh, sw, ph0, pw0; };

// device memory of a graph comes out of a few large allocations (bump-allocated, 256-byte granules): one hipMalloc per tensor /
// weight blob scatters a model over hundreds of separately mapped ranges, and inside a pass every launch then starts with
// translation misses on pages it last touched a whole step ago
struct DevArena { char* base = nullptr; size_t cap = 0, used = 0; };

}  // namespace tamd

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            tamd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return -1;                                                                            \
        }                                                                                         \
    } while (0)

struct tamd_graph {
    // "one graph = one thread at a time" (include/tengine_amd.h), enforced: the token of the thread inside a call that changes the graph
    // or touches its buffers (0: nobody).  A second thread's call fails with an error instead of racing (graph_internal.h: OneThread)
    std::atomic<unsigned long> owner{0};
    std::vector<tamd::HTensor> tensors;
    std::vector<tamd::HNode> nodes;
    std::vector<tamd::IOBind> inputs, outputs;
    std::vector<tamd::Step> steps;      // compute launches
    std::vector<tamd::Step> in_steps;   // input layout launches (after H2D)
    std::vector<tamd::Step> out_steps;  // output layout launches (before D2H)
    std::vector<void*> dev_allocs;
    std::vector<tamd::DevArena> arenas;       // dev_alloc(): bump allocation out of these (each is also in dev_allocs)
    std::vector<char> pooled;           // tensors whose buffer is shared with other tensors of disjoint lifetime (read_tensor refuses them)
    size_t pool_bytes = 0, unpooled_bytes = 0;     // activation arena with / without lifetime sharing (TAMD_DEBUG prints both)
    std::map<int, float*> f32_copy;     // uint8 tensor -> its dequantised fp32 copy (input of the fp32 MFMA conv kernel)
    std::vector<char> fused_away;       // tensors that only exist inside a fused launch (read_tensor refuses them)
    void* zero_page = nullptr;          // 256 zero bytes (out-of-image taps of the LDS-DMA conv kernel)
    hipStream_t stream = nullptr;
    hipGraph_t hgraph = nullptr;
    hipGraphExec_t hexec = nullptr;     // == hexecs[0]
    // several instances of the same captured graph, launched round-robin: back-to-back replays of ONE hipGraphExec_t
    // leave a ~9 us hole between them on the device (the next launch is not queued behind the running one); with
    // independent instances the next replay's packets are already in the queue (profiles/r02_*replay*)
    hipGraphExec_t hexecs[4] = {nullptr, nullptr, nullptr, nullptr};
    int nexec = 0, next_exec = 0;
    tamd::IoSlot io[2];                        // host-to-host runs (tamd_graph_run / _run_async): the two I/O slots
    int next_io_slot = 0;                      // the I/O slot of the next tamd_graph_run_async
    std::vector<tamd::Inflight> inflight;      // FIFO, at most 2
    tamd::DirectProgram* direct = nullptr;     // tamd_options.direct_dispatch: the launch list as AQL packets (direct.cc)
    // two pass slots (graph_slots.hip): a second program of the SAME launch list on an HSA queue of its own, its written buffers re-pointed
    // at a private copy (slot_block); tamd_graph_launch alternates between the two, so two passes are in flight.  nullptr: one list
    tamd::DirectProgram* direct1 = nullptr;
    void* slot_block = nullptr;                // slot 1's copy of everything a pass writes (one allocation)
    std::vector<tamd::SlotSpan> slot_spans;    // where each written span of slot 0 lives in it
    int slot_turn = 0;                         // whose turn the next tamd_graph_launch is; direct_drain sets it back to 0
    bool slot_hold = false;                    // tamd_graph_time_launches: slot 0 alone (the pass as the dependent chain it is)
    bool had_once = false;                     // the plan held launches that ran once at prerun (their results exist in slot 0 only)
    int autotune_cold = -1;                    // plan-time timing mode, decided once (autotune_cold())
    double prerun_ms = 0;                      // wall time of tamd_graph_prerun (planning, autotune, capture)
    bool direct_busy = false;                  // passes submitted since the last wait
    bool stream_dirty = true;                  // something may be pending on `stream` (uploads, eager launches): drain it before a direct burst
    bool stream_exposed = false;               // tamd_graph_stream() handed the stream out: the caller may queue work this library cannot see
    int out_fresh_in = -1;                     // -1: the outputs' device staging buffers hold the last pass; 0 / 1: only the pinned buffers of that
                                               // I/O slot do (a zero-copy host-to-host run): stage_from_pinned() before anything reads the device copy
    // TAMD_H2H_TRACE=1: where a blocking tamd_graph_run spends its time on the host (ns): copy in, stream drain, submit, wait, copy out
    long long h2h_ns[5] = {0, 0, 0, 0, 0};
    long long h2h_runs = 0;
    tamd_options opt{};
    bool prepared = false;
    int gpu = 0;
    // round 6: a batched graph of batch-wise independent operators is compiled as TWO device graphs of half the batch each
    // (graph_pair.hip): half[0] runs images [0, B / 2), half[1] the rest, side by side on their own HSA queues.  This object then
    // keeps the IR (descriptions, constants) and forwards every entry point; it owns no stream, launch list or device tensor.
    tamd_graph* half[2] = {nullptr, nullptr};
    bool is_half = false;                      // one of the two halves of such a pair: never split again
    // ... and the batch of the WHOLE graph it is a part of (0: its own).  The reference picks the formula of a 3x3 depthwise
    // convolution by batch == 1 (conv_dw_hcl_x86.c:508-543 score(): the hand-written kernel at batch 1, ref_conv_int8 otherwise --
    // another requantisation chain, graph_plan_conv.hip: conv_mode): the halves of a 2-image graph run ONE image each and must still
    // produce the 2-image graph's bytes (found by tools/fuzz_split.py: 7 of 931 graphs differed before this field existed)
    int formula_batch = 0;
    std::vector<void*> pair_out;               // tamd_graph_output_device of a pair: the two halves gathered into one buffer per output
};

namespace tamd {

// planner helpers shared by graph_plan.hip (int8, NHWC), graph_u8.hip (uint8, NCHW) and graph_f32.hip (fp32, NCHW): graph_plan_common.hip
PoolGeom pool_geom(const tamd_pool_param& p, int h, int w);
int dev_alloc(tamd_graph* g, void** p, size_t bytes, bool zero);
// plan-time races (plan_cache.hip).  A candidate: the plan-cache tag that names it, how to launch it (one launch, or several
// back to back: the two unfused steps of a pair, the three Winograd launches), the kernel name TAMD_DEBUG prints (empty: the
// tag) and whether a cached tag may still pick it (unset: yes; a pinned site answers no, it never reads the plan file).
struct RaceCand {
    std::string tag;
    std::function<hipError_t(hipStream_t)> fn;
    std::string name;
    std::function<bool()> live;
};
// plan_race: the winner's index.  cands[0] is the incumbent (the heuristic choice; also the answer when `tune` is false); a
// candidate that does not launch is skipped; a later one wins when it beats the best so far by `margin` (ms < best * margin), so
// in an ordered list the last to do so wins.  A non-empty `key` is looked up in the plan cache first (TAMD_PLAN_CACHE: a tag that
// names a live candidate answers without timing) and gets the winner's tag; an empty key neither reads nor writes.  -1: HIP error.
int plan_race(tamd_graph* g, const std::string& node, const std::vector<RaceCand>& cands, const std::string& key, float margin, bool tune);
// the lookup alone: the index of the live candidate whose tag the cached entry of `key` holds, -1: none
int plan_cached(const std::string& key, const std::vector<RaceCand>& cands);
bool autotune_enabled();           // TAMD_AUTOTUNE=0: no site races, every one keeps its incumbent
void nhwc_geom(HTensor& t);
// The one place a launch goes onto g->steps, for all three planners: refuses, at the node that planned it, a launch that states no read
// or no write and one whose write overlaps its own read
int append_steps(tamd_graph* g, const std::vector<Step>& launches);
int count_consumers(const tamd_graph* g, int tensor);
// the front and the tail that the NCHW planners (graph_u8.hip, graph_f32.hip) share: dense buffers of `esz` bytes per element for
// inputs and tensors, views for Dropout / Flatten / Reshape and for channel-concat inputs that `in_place` allows; graph outputs
int plan_nchw_buffers(tamd_graph* g, size_t esz, const std::function<bool(const HNode& producer, const HTensor& x, const HTensor& cat)>& in_place);
int plan_nchw_outputs(tamd_graph* g, size_t esz);
// The byte-map node planners that both quantised graphs call (graph_plan_maps.hip); each hands its launches back in *out.
// a Sigmoid / Clip / HardSwish / Mish node of an int8 or uint8 graph as ONE launch: table upload + lut_u8
int plan_lut(tamd_graph* g, HNode& n, std::vector<Step>* out);
// a nearest Interp node of an int8 (NHWC) or uint8 (NCHW) graph as ONE launch: index vectors and byte map uploaded,
// interp_nearest_i8 / interp_nearest_u8; reads and writes channel slices (concat views)
// crop (uint8 graphs; crop_interp_producer): the Crop that alone reads the Interp runs inside the launch -- the index vectors shifted and
// cut by its box, the Crop's output written, the Interp's own output never
int plan_interp(tamd_graph* g, HNode& n, std::vector<Step>* out, const HNode* crop = nullptr);
// Split / ShuffleChannel of a uint8 (NCHW) graph: one chan_map_u8 launch per output tensor, the plane map and the
// Split's byte map uploaded.  The int8 forms are declared in graph_plan.h
int plan_split_u8(tamd_graph* g, HNode& n, std::vector<Step>* out);
int plan_shuffle_u8(tamd_graph* g, HNode& n, std::vector<Step>* out);
// a PReLU node of an int8 (NHWC) or uint8 (NCHW) graph as ONE launch: the slopes widened (int8) or one byte table per
// channel built (uint8) and uploaded, prelu_i8 / prelu_u8 (prelu.hip)
int plan_prelu(tamd_graph* g, HNode& n, std::vector<Step>* out);
// prelu_refusal (node_rules.h) asked of a node of this graph, payload included: validate_graph and plan_prelu
const char* prelu_refusal_of(const tamd_graph* g, const HNode& n);
// slice_refusal (node_rules.h) asked of a node of this graph: infer_shapes (check_out false: the output's dims are not made yet),
// validate_graph and plan_slice_u8.  *geom / table[256] (either may be null): the resolved box and the byte map
const char* slice_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, SliceGeom* geom, unsigned char* table);
// the Slice that can run inside the launch of Slice `ni` (a chain of two as one slice_u8 launch): the one reader of its output, which
// is no graph output; both nodes pass slice_refusal; TAMD_PIN=slice_chain=0 is not set.  Its node index, -1: none
int slice_chain_next(const tamd_graph* g, size_t ni);
// a Slice node of a uint8 (NCHW) graph as ONE slice_u8 launch (slice.hip); with next >= 0 that Slice too: boxes and byte maps
// composed, the tensor between them fused away
int plan_slice_u8(tamd_graph* g, HNode& n, int next, std::vector<Step>* out);
// transpose_refusal (node_rules.h) asked of a node of this graph: infer_shapes (check_out false: the output's dims are not made yet),
// validate_graph and plan_transpose.  *geom / table[256] (either may be null): the canonical geometry for a dense input and the byte map
const char* transpose_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, TransposeGeom* geom, unsigned char* table);
// the strides under which `dims` index the convolution-stack NHWC buffer of s, where every axis factors one of s's N, C, H * W ranges
bool nhwc_view_strides(const HTensor& s, const std::vector<int>& dims, long* strides);
// a Transpose node of an int8 or uint8 graph as ONE launch (transpose.hip); view_src >= 0: read through the Reshape in front of it
int plan_transpose(tamd_graph* g, HNode& n, int view_src, std::vector<Step>* out);
// crop_refusal (node_rules.h) asked of a node of this graph: infer_shapes (check_out false: the output's dims are not made yet),
// validate_graph and the planners.  *geom (may be null): the resolved box
const char* crop_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, CropGeom* geom);
// the nearest Interp that can run inside the launch of Crop `ci` (Interp -> Crop as one interp_nearest_u8 launch): it makes the Crop's
// data input, which nothing else reads and which is no graph output or view; it passes interp_refusal, the Crop passes crop_refusal and
// its box cuts no channels; TAMD_PIN=crop_chain=0 is not set.  Its node index, -1: none
int crop_interp_producer(const tamd_graph* g, size_t ci);
// the same-shape Eltwise (PROD, SUM, SUB, MAX) that can take the Interp -> Crop chain of Crop `ci` into ITS launch (topdown_u8): the one
// reader of the Crop's output, which is no graph output; its other operand a dense tensor of the output's dims;
// crop_interp_producer(ci) >= 0 and TAMD_PIN=topdown=1 is set (opt-in: measured level with or behind the two launches it replaces,
// profiles/crop_topdown.txt).  Its node index, -1: none
int crop_topdown_next(const tamd_graph* g, size_t ci);
// a Crop node of a uint8 (NCHW) graph alone: ONE slice_u8 launch over the box in its identity form (raw bytes, step 1)
int plan_crop_u8(tamd_graph* g, HNode& n, std::vector<Step>* out);
// Interp `in` -> Crop `cn` -> Eltwise `n` as ONE topdown_u8 launch (topdown.hip), planned at the Eltwise's position
int plan_topdown_u8(tamd_graph* g, HNode& in, HNode& cn, HNode& n, std::vector<Step>* out);
// depthtospace_refusal (node_rules.h) asked of a node of this graph: infer_shapes (check_out false: the output's dims are not made yet),
// validate_graph and the planners.  *geom (may be null): the block size, the output's dims, the six-axis view
const char* depthtospace_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, DepthToSpaceGeom* geom);
// a DepthToSpace node of an int8 (NHWC) or uint8 (NCHW) graph as ONE launch: d2s_i8 / d2s_u8 (d2s.hip), or with TAMD_PIN=d2s_form=0, where
// the output is one dense run, the canonical gather of transpose.hip with the identity map.  fix128 (int8): the output lies in the
// buffer of a Concat of several inputs, whose copy stores 127 for the byte -128
int plan_depthtospace(tamd_graph* g, HNode& n, bool fix128, std::vector<Step>* out);
// resize_refusal (node_rules.h) asked of a node of this graph: infer_shapes (check_out false: the output's dims are not made yet),
// validate_graph and the planners.  *geom (may be null): the output's dims, the two index vectors, the byte map, the whole-number factors
const char* resize_refusal_of(const tamd_graph* g, const HNode& n, bool check_out, ResizeGeom* geom);
// a nearest Resize node of an int8 (NHWC) or uint8 (NCHW) graph as ONE launch.  Form 0: interp_nearest_i8 / interp_nearest_u8 (interp.hip)
// fed with Resize's index vectors and table, legal for every accepted node.  Form 1: resize_rep_i8 / resize_rep_u8 (resize.hip), legal
// at whole-number factors (ResizeGeom::sh / sw).  TAMD_PIN=resize_form=0|1 chooses; the output's size otherwise (kernels.h: kResizeRepFromBytesU8 / I8)
int plan_resize(tamd_graph* g, HNode& n, std::vector<Step>* out);
// eltwise_refusal (node_rules.h) asked of a node of this graph: validate_graph and the int8 / uint8 Eltwise planners.  *gated: -1 the
// same-shape form, 0 | 1 which input is x of the channel-gate form x (N, C, H, W) op gate (N, C, 1, 1), kEltScalar / kEltUnary the two
// forms that run by table; table[256]: the byte map of those two (may be null)
const char* eltwise_refusal_of(const tamd_graph* g, const HNode& n, int* gated, unsigned char* table = nullptr);
// batchnorm_refusal (node_rules.h) asked of a node of this graph, payloads included: validate_graph and plan_batchnorm_u8.  tables (may be
// null): the [C][64] dwords of the C byte maps
const char* batchnorm_refusal_of(const tamd_graph* g, const HNode& n, std::vector<unsigned>* tables);
// a BatchNorm node of a uint8 graph as ONE launch through its C byte maps: chan_lut_u8 (chan_lut.hip), or prelu_u8's per-plane form
// (prelu.hip) on planes of at least kBnPlaneForm bytes; TAMD_PIN=bn_form=0 | 1 forces the first | the second
int plan_batchnorm_u8(tamd_graph* g, HNode& n, std::vector<Step>* out);
// instancenorm_refusal (node_rules.h) asked of a node of this graph, gamma / beta payloads included: validate_graph and plan_instancenorm_u8
const char* instancenorm_refusal_of(const tamd_graph* g, const HNode& n);
// the plain or leaky ReLU that is the only reader of InstanceNorm node ni's output (no graph output) and is composed into the plane's
// map, -1: none (or TAMD_PIN=instnorm_relu=0); which form runs on planes of that many bytes: 0 instnorm_stats_u8 + chan_lut_u8, 1 instnorm_u8
// (TAMD_PIN=instnorm_form; the measured default is in graph_plan_maps.hip)
int instancenorm_relu_next(const tamd_graph* g, size_t ni);
int instancenorm_form(size_t plane_bytes);
// an InstanceNorm node of a uint8 graph (instnorm.hip), `relu` (may be null) inside: two launches or one
int plan_instancenorm_u8(tamd_graph* g, HNode& n, const HNode* relu, std::vector<Step>* out);
// the scalar and the unary Eltwise, int8 and uint8 graphs alike: one lut_u8 launch through tamd_eltwise_table's bytes
int plan_eltwise_table(tamd_graph* g, HNode& n, std::vector<Step>* out);
// A byte-pure chain (graph_plan_maps.hip): nodes[] in node order, each a table node (Sigmoid / Clip / HardSwish / Mish, scalar or unary
// Eltwise) behind `src` or a member, or a same-shape Eltwise whose operands are `src` or members, and each one that `last`, the last
// member's output, depends on; table: the byte of `last` for every byte of `src`.  The outputs of all members but the last have no reader outside the chain and are no graph
// outputs.
struct ByteChain {
    int src = -1, last = -1;
    std::vector<int> nodes;
    unsigned char table[256];
};
// the maximal chain of at least two nodes that starts at table node `ni`, false: none (or TAMD_PIN=bytemap_chain=0).  node_free(node):
// the planner has not given the node to another launch; tensor_plain(tensor): it owns a whole buffer in the layout of its neighbours
// (no view, no alias, not dense among NHWC tensors) -- what only a planner knows stays with that planner
bool bytemap_chain_from(const tamd_graph* g, size_t ni, const std::function<bool(int)>& node_free, const std::function<bool(int)>& tensor_plain, ByteChain* c);
// the chain as ONE lut_u8 launch from src to last, planned at the LAST member's position; the tensors between are fused away
int plan_bytemap_chain(tamd_graph* g, const ByteChain& c, std::vector<Step>* out);
// the byte-map node (Sigmoid / Clip / HardSwish / Mish) that produces the gate of the channel-gate Eltwise `e` and can run inside
// its launch -- the gate has no other reader, is no graph output and no view, TAMD_PIN=gate_lut=0 is not set --, -1: none.  What
// only a planner knows of its layout (int8: dense / view bookkeeping before the buffers exist) stays with that planner
int gate_lut_producer(const tamd_graph* g, const HNode& e, int gated);
// a channel-gate Eltwise of an int8 (NHWC) or uint8 (NCHW) graph as ONE launch: chan_gate_i8 / chan_gate_u8 (chan_gate.hip); with
// lut_node >= 0 that node's byte table is uploaded and applied to the gate bytes in the same launch (lut_chan_gate_*), its output
// tensor is fused away
int plan_chan_gate(tamd_graph* g, HNode& n, int gated, int lut_node, std::vector<Step>* out);
// output placement of a dense NCHW tensor: elements per image of the buffer it lives in (a concat slice when it is a view; first channel: c_off)
inline int nchw_out_img(const HTensor& t) { return (t.is_view ? t.cs : t.c) * t.h * t.w; }
// .. and the small things their node planners share.  A softmax / concat axis (negative: from the back) as [outer][on][inner] of
// dense `dims`; -1 and the error "<what> <node>: bad axis" when it names no dimension
struct AxisSplit { int axis = 0, outer = 1, on = 0, inner = 1; };
int axis_split(const std::vector<int>& dims, int axis, const char* what, const std::string& node, AxisSplit* s);
// [Kpad] packed tap table of a group-1 convolution, k = (c, ky, kx): (c*H*W + ky*DH*W + kx*DW) | kx*DW << 24 | ky*DH << 28; padding 0
std::vector<unsigned> conv_tap_table(int K, int Kpad, int H, int W, int KH, int KW, int DH, int DW);
int priorbox_count(const tamd_priorbox_param& p);
void priorbox_eval(const tamd_priorbox_param& p, int feat_h, int feat_w, int data_h, int data_w, std::vector<float>* out);
void priorbox_quant_u8(const std::vector<float>& f, float scale, int zp, std::vector<uint8_t>* q);
void priorbox_quant_i8(const std::vector<float>& f, float scale, std::vector<int8_t>* q);
int plan_u8(tamd_graph* g);        // graph_u8.hip: every activation tensor is uint8
int plan_f32(tamd_graph* g);       // graph_f32.hip: every activation tensor is fp32

template <typename T>
int upload(tamd_graph* g, const std::vector<T>& host, T** dev)
{
    void* p = nullptr;
    if (dev_alloc(g, &p, host.size() * sizeof(T), false)) return -1;
    HIPCHK(hipMemcpyAsync(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, g->stream));   // own stream only
    HIPCHK(hipStreamSynchronize(g->stream));
    *dev = (T*)p;
    return 0;
}

// the first n elements of a bias tensor on the device; no tensor: *dev stays null
template <typename T>
int upload_bias(tamd_graph* g, const HTensor* b, int n, const T** dev)
{
    if (!b) return 0;
    std::vector<T> hb((const T*)b->data.data(), (const T*)b->data.data() + n);
    T* d = nullptr;
    if (upload(g, hb, &d)) return -1;
    *dev = d;
    return 0;
}

// the constant operands of conv_f32_mfma for the geometry in `a`: picks the tile configuration (a.cfg), uploads the weights in its
// layout -- [cout tile of BM][stage of 32 k][group][ (k%G)*BM + c ], G = 64 / BM k rows per 64-float group, zero padded -- and
// the tap table (a.w, a.klut).  wk(co, k): weight k of output channel co as float
template <typename F>
int conv_f32_mfma_operands(tamd_graph* g, F32ConvArgs& a, int KH, int KW, int DH, int DW, F wk)
{
    a.cfg = conv_f32_mfma_pick(a);
    const int BM = conv_f32_mfma_bm(a.cfg), ntile = (a.cout + BM - 1) / BM, nstage = a.Kpad / 32, G = 64 / BM, NIg = 32 / G;
    std::vector<float> wf((size_t)ntile * nstage * 32 * BM, 0.f);
    for (int co = 0; co < a.cout; co++)
        for (int k = 0; k < a.K; k++) {
            const int r = k & 31;
            wf[(((size_t)(co / BM) * nstage + (k >> 5)) * NIg + r / G) * 64 + (r % G) * BM + co % BM] = wk(co, k);
        }
    float* dwf = nullptr; unsigned* dlut = nullptr;
    if (upload(g, wf, &dwf) || upload(g, conv_tap_table(a.K, a.Kpad, a.H, a.W, KH, KW, DH, DW), &dlut)) return -1;
    a.w = dwf; a.klut = dlut;
    return 0;
}

}  // namespace tamd
