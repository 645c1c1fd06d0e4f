// What every planner shares (graph_plan.hip int8, graph_u8.hip uint8, graph_f32.hip fp32): device memory (dev_alloc), tensor geometry,
// the front and the tail of the two NCHW planners, the small helpers of their node functions, and append_steps -- the one place a
// launch goes onto g->steps.  Declared under "planner helpers shared by ..." in graph.h.
#include "graph.h"
#include "graph_internal.h"
#include "env.h"

#include <algorithm>

namespace tamd {

int dev_alloc(tamd_graph* g, void** p, size_t bytes, bool zero)
{
    // slack: the pointwise kernels read whole 64-byte K steps, up to 8 of them past a pixel row's last channel (those
    // bytes meet zero weights, but must be readable behind the last pixel of a buffer too)
    const size_t slack = 1024;
    const char* ae = tamd_pin("arena");                       // 0: one hipMalloc per buffer (round 1-3 behaviour; A/B runs)
    if (ae && atoi(ae) == 0) {
        HIPCHK(hipMalloc(p, bytes + slack));
        g->dev_allocs.push_back(*p);
        if (zero) HIPCHK(hipMemsetAsync(*p, 0, bytes + slack, g->stream));    // never the legacy stream: it would collide with another thread's capture
        return 0;
    }
    // bump allocation out of a few large chunks: a model's tensors, weights and per-channel vectors are hundreds of buffers, and
    // as separate hipMalloc ranges each brings its own page-table fragment -- inside a pass every launch then begins with
    // translation misses on memory it last touched a step ago.  One contiguous range per 32 MB .. 1 GB maps with large fragments.
    const size_t need = (bytes + slack + 255) & ~(size_t)255;
    DevArena* a = g->arenas.empty() ? nullptr : &g->arenas.back();
    if (!a || a->used + need > a->cap) {
        size_t cap = g->arenas.empty() ? ((size_t)32 << 20) : std::min<size_t>(2 * g->arenas.back().cap, (size_t)1 << 30);
        cap = (std::max(cap, need) + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
        DevArena na;
        HIPCHK(hipMalloc((void**)&na.base, cap));
        na.cap = cap;
        g->dev_allocs.push_back(na.base);
        g->arenas.push_back(na);
        a = &g->arenas.back();
    }
    *p = a->base + a->used;
    a->used += need;
    if (zero) HIPCHK(hipMemsetAsync(*p, 0, bytes + slack, g->stream));
    return 0;
}

void nhwc_geom(HTensor& t)
{
    if (t.dims.size() == 4) { t.n = t.dims[0]; t.c = t.dims[1]; t.h = t.dims[2]; t.w = t.dims[3]; }
    else if (t.dims.size() == 2) { t.n = t.dims[0]; t.c = t.dims[1]; t.h = t.w = 1; }
    else { t.n = 1; t.c = (int)t.elems(); t.h = t.w = 1; }
}

// The NCHW planners' front: every non-constant tensor is dense NCHW bytes (read_tensor / IO copy them as they are), `esz` bytes per
// element.  Allocation order: the graph inputs in their order, then every remaining tensor that owns a buffer in index order.
// concat-by-offset: a node whose only consumer is a channel concat writes its channels straight into the concat
// output, and the concat launch disappears, where in_place(producer, input, concat output) says that it may.
int plan_nchw_buffers(tamd_graph* g, size_t esz, const std::function<bool(const HNode& producer, const HTensor& x, const HTensor& cat)>& in_place)
{
    for (auto& t : g->tensors) {
        if (t.ttype == TAMD_TT_CONST) continue;
        nhwc_geom(t);
        t.nchw_raw = true;
        t.cs = 0; t.c_off = 0;
    }
    std::vector<int> alias_of(g->tensors.size(), -1);
    for (auto& n : g->nodes)
        if (n.op == TAMD_OP_DROPOUT || n.op == TAMD_OP_FLATTEN || n.op == TAMD_OP_RESHAPE) alias_of[n.out[0]] = n.in[0];   // dense NCHW: views
    for (auto& io : g->inputs) {
        HTensor& t = g->tensors[io.tensor];
        io.bytes = t.elems() * esz;
        if (dev_alloc(g, &io.stage, io.bytes, true)) return -1;
        t.dptr = io.stage;
    }
    std::vector<int> view_of(g->tensors.size(), -1), view_off(g->tensors.size(), 0);
    for (auto& n : g->nodes) {
        if (n.op != TAMD_OP_CONCAT) continue;
        HTensor& y = g->tensors[n.out[0]];
        const int ax = n.p.concat.axis < 0 ? n.p.concat.axis + (int)y.dims.size() : n.p.concat.axis;
        int off = 0;
        for (int i : n.in) {
            HTensor& xi = g->tensors[i];
            bool ok = ax == 1 && xi.ttype == TAMD_TT_VAR && count_consumers(g, i) == 1 && alias_of[i] < 0 && view_of[i] < 0;
            if (ok) {
                ok = false;
                for (auto& pn : g->nodes)
                    if (!pn.out.empty() && pn.out[0] == i) ok = in_place(pn, xi, y);
            }
            if (ok) { view_of[i] = n.out[0]; view_off[i] = off; }
            off += xi.c;
        }
    }
    for (size_t i = 0; i < g->tensors.size(); i++) {
        HTensor& t = g->tensors[i];
        if (t.ttype == TAMD_TT_CONST || t.dptr || alias_of[i] >= 0 || view_of[i] >= 0) continue;
        if (dev_alloc(g, &t.dptr, t.elems() * esz, true)) return -1;
    }
    for (size_t i = 0; i < g->tensors.size(); i++)
        if (view_of[i] >= 0) {
            HTensor& t = g->tensors[i];
            HTensor& o = g->tensors[view_of[i]];
            if (!o.dptr) { set_error("concat of concat views is not supported"); return -1; }
            t.dptr = o.dptr; t.is_view = true; t.c_off = view_off[i]; t.cs = o.c;      // cs: channels of the enclosing buffer
        }
    for (int pass = 0; pass < 4; pass++)
        for (size_t i = 0; i < g->tensors.size(); i++)
            if (alias_of[i] >= 0) g->tensors[i].dptr = g->tensors[alias_of[i]].dptr;
    return 0;
}

int plan_nchw_outputs(tamd_graph* g, size_t esz)
{
    for (auto& io : g->outputs) {
        HTensor& t = g->tensors[io.tensor];
        io.bytes = t.elems() * esz;
        io.stage = t.dptr;
    }
    return 0;
}

int count_consumers(const tamd_graph* g, int tensor)
{
    int c = 0;
    for (auto& n : g->nodes)
        for (int i : n.in) c += (i == tensor);
    for (auto& o : g->outputs) c += (o.tensor == tensor);
    return c;
}

int axis_split(const std::vector<int>& dims, int axis, const char* what, const std::string& node, AxisSplit* s)
{
    const int ax = axis < 0 ? axis + (int)dims.size() : axis;
    if (ax < 0 || ax >= (int)dims.size()) { set_error("%s %s: bad axis", what, node.c_str()); return -1; }
    *s = AxisSplit{};
    s->axis = ax; s->on = dims[ax];
    for (int d = 0; d < ax; d++) s->outer *= dims[d];
    for (size_t d = ax + 1; d < dims.size(); d++) s->inner *= dims[d];
    return 0;
}

std::vector<unsigned> conv_tap_table(int K, int Kpad, int H, int W, int KH, int KW, int DH, int DW)
{
    std::vector<unsigned> lut(Kpad, 0u);
    for (int k = 0; k < K; k++) {
        const int kx = k % KW, ky = (k / KW) % KH, c = k / (KW * KH);
        lut[k] = (unsigned)(c * H * W + ky * DH * W + kx * DW) | (unsigned)(kx * DW) << 24 | (unsigned)(ky * DH) << 28;
    }
    return lut;
}

// The one place a launch goes onto g->steps, for plan_i8, plan_u8 and plan_f32.  Every compute launch reads and writes some activation
// and says so (graph.h: make_step), and a launch that writes what it reads is an error.  In an int8 graph a fused launch runs at its
// first node's position -- chain4 and ReLU + pool even ahead of node order, a convolution's eltwise tail and eltwise + ReLU a node or
// two ahead -- and writes its output while other blocks still read its input; only plan_buffers' birth rule keeps the two out of one
// shared buffer.  The NCHW planners share no buffers yet; the day they do, the same check holds them to it
int append_steps(tamd_graph* g, const std::vector<Step>& launches)
{
    for (auto& st : launches) {
        if (step_states_nothing(st)) {
            set_error("launch %s (%s) does not state what it reads and writes", st.kernel.c_str(), st.node.c_str());
            return -1;
        }
        if (step_writes_what_it_reads(st)) {
            set_error("launch %s (%s) writes memory that it reads: its output shares a buffer with its input", st.kernel.c_str(), st.node.c_str());
            return -1;
        }
        g->steps.push_back(st);
    }
    return 0;
}

}  // namespace tamd
